"""The reference's coordinate_conversion.py (:4-61): cell index <-> (alpha, beta) angle <-> point on the unit sphere.

Scalar helpers on the host, like vp_localisation.line_length: NumPy float64 with the reference's order of operations, so
the values are the reference's to the last bit.  ``angles_to_indices`` is the row-wise form of ``angle_to_index`` that the
overlay renderer (result_plotting.py) places its markers with."""
import numpy as np


def index_to_angle(index, shape):
    """:4-20: the angle at the centre of cell ``index`` of an M x N grid over [-pi/2, pi/2]^2."""
    angle = np.zeros(2)
    a = index[0]
    b = index[1]
    M = shape[0]
    N = shape[1]
    angle[0] = (a - 0.5 * M + 0.5) * np.pi / M
    angle[1] = (b - 0.5 * N + 0.5) * np.pi / N
    return angle


def angle_to_index(angle, shape):
    """:23-35: the (fractional) cell index of ``angle``; the inverse of index_to_angle."""
    alpha = angle[0]
    beta = angle[1]
    M = shape[0]
    N = shape[1]
    a = (alpha / np.pi + 0.5 - 0.5 / M) * M
    b = (beta / np.pi + 0.5 - 0.5 / N) * N
    return np.array([a, b])


def angles_to_indices(angles, shape):
    """angle_to_index for every row of an (M, 2) array: the same arithmetic, row by row."""
    angles = np.asarray(angles, dtype=np.float64).reshape(-1, 2)
    out = np.zeros(angles.shape)
    for j in range(angles.shape[0]):
        out[j] = angle_to_index(angles[j], shape)
    return out


def angle_to_point(angle):
    """:38-50: the unit vector of ``angle``, flipped into z >= 0 (:48; np.sign(0) = 0 gives the zero vector at z == 0)."""
    alpha = angle[0]
    beta = angle[1]
    point = np.zeros(3)
    point[1] = np.sin(beta)
    point[0] = np.sin(alpha) * np.cos(beta)
    point[2] = np.cos(alpha) * np.cos(beta)
    point *= np.sign(point[2])
    return point


def point_to_angle(point):
    """:53-61: (alpha, beta) of a unit vector; the quotient is clamped to [-1, 1] in front of the arcsin (:57-58)."""
    angle = np.zeros(2)
    angle[1] = np.arcsin(point[1])
    inner = point[0] / np.cos(angle[1])
    inner = np.minimum(inner, 1)
    inner = np.maximum(inner, -1)
    angle[0] = np.arcsin(inner)
    return angle
