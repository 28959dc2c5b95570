"""Ground truth of the three benchmark datasets -- the reference's benchmark.py:81-99 and :137-220 as functions.

York Urban (YUD): three orthogonal VPs per image in a .mat file, brought to the normalised frame through the camera
matrix.  Eurasian Cities (ECD): zenith, horizon VPs and the horizon line in pixel coordinates.  Horizon Lines in the Wild
(HLW): two horizon end points per image in metadata.csv.  All three end in a horizon line in the frame the detector works
in (x, y in [-1, 1] along the longer side, y up), which calc_horizon.horizon_error compares a detected horizon with.

The reference is Python 2 without `from __future__ import division`: where both operands of its `/` are integers the
division floors, and this port writes `//` there (ECD: imageWidth/2, imageHeight/2 and scale/2, :180-183).  That is part
of the ground truth of every ECD image with an odd side.  The .mat files are read with scipy.io.loadmat like the
reference's; SciPy is imported inside the loaders, so the package imports without it."""
import csv
import os

import numpy as np


def _loadmat(path):
    try:
        from scipy import io
    except ImportError as e:
        raise ImportError("the ground truth of the YUD and ECD datasets is stored in .mat files: reading %s needs "
                          "scipy.io.loadmat (SciPy is not installed)" % path) from e
    return io.loadmat(path)


def york_camera(source_folder):
    """benchmark.py:82-89: (K, S) from <source_folder>/cameraParameters.mat.  K maps a direction to pixels around the
    principal point the reference hard-codes (13, -11), S scales pixels by 2 / 640."""
    params = _loadmat(os.path.join(source_folder, "cameraParameters.mat"))            # :82
    f = params['focal'][0, 0]                                                          # :84
    ps = params['pixelSize'][0, 0]                                                     # :85
    fp = f // ps if all(np.issubdtype(np.asarray(x).dtype, np.integer) for x in (f, ps)) else f / ps
    K = np.array([[fp, 0, 13], [0, fp, -11], [0, 0, 1]], dtype=np.float64)             # :88
    S = np.array([[2.0 / 640, 0, 0], [0, 2.0 / 640, 0], [0, 0, 1]])                    # :89
    return K, S


def york_truth(image_file, K, S):
    """benchmark.py:128-167 for <dir>/<ID>/<ID>.jpg: reads <dir>/<ID>/<ID>GroundTruthVP_CamParams.mat (`vp`: 3 x 3, VPs in
    columns).  Returns (true_vps 3 x 3 with the VPs in rows, true_horizon = cross(tVP1, tVP3))."""
    basename = os.path.splitext(image_file)[0]                                         # :128
    path0, image_id = os.path.split(basename)                                          # :134
    path1, _ = os.path.split(path0)                                                    # :135
    gt = _loadmat("%s/%s/%sGroundTruthVP_CamParams.mat" % (path1, image_id, image_id))  # :143-145
    vps = np.dot(K, np.array(gt['vp'], dtype=np.float64))                              # :147-150
    for c in range(3):
        vps[:, c] /= vps[2, c]                                                         # :152-154
    vps = np.dot(S, vps)                                                               # :156
    rows = []
    for c in range(3):
        v = np.array(vps[:, c])
        v /= v[2]                                                                      # :158-163
        rows.append(v)
    return np.vstack(rows), np.cross(rows[0], rows[2])                                 # :165-167


def eurasian_truth(image_file, width, height):
    """benchmark.py:128, :137, :171-203 for an image of width x height pixels: reads <base>VP.mat (`zenith` 1 x 2,
    `hor_points` K x 2, pixels) and <base>hor.mat (`horizon`, 3 values in either orientation).  Returns
    (true_vps (K + 1) x 3 with the zenith first, true_horizon)."""
    width, height = int(width), int(height)
    basename = os.path.splitext(image_file)[0]
    scale = max(width, height)                                                         # :137
    vp_mat = _loadmat("%sVP.mat" % basename)                                           # :172-175
    zenith, hor_vps = vp_mat['zenith'], vp_mat['hor_points']
    vps = np.ones((hor_vps.shape[0] + 1, 3))                                           # :177
    vps[:, 0:2] = np.vstack([zenith, hor_vps])
    vps[:, 0] -= width // 2                                                            # :180  int / int
    vps[:, 1] -= height // 2                                                           # :181  int / int
    vps[:, 1] *= -1
    vps[:, 0:2] /= scale // 2                                                          # :183  int / int
    horizon = np.squeeze(_loadmat("%shor.mat" % basename)['horizon'])                  # :185-186
    p1 = np.cross(horizon, np.array([-1, 0, width]))                                   # :188
    p2 = np.cross(horizon, np.array([-1, 0, 0]))
    p1 = p1 / p1[2]                                                                    # :190-191
    p2 = p2 / p2[2]
    for p in (p1, p2):
        p[0] -= width / 2.0                                                            # :193-196
        p[1] -= height / 2.0
        p[1] *= -1                                                                     # :197-198
        p[0:2] /= scale / 2.0                                                          # :200-201
    return vps, np.cross(p1, p2)                                                       # :203


def horizon_metadata(source_folder):
    """benchmark.py:93-99: the rows of <source_folder>/metadata.csv, the first field cut down to the file's base name
    (no directory, nothing from the first dot on).  Text mode: the reference's 'rb' is Python 2's."""
    rows = []
    with open(os.path.join(source_folder, "metadata.csv"), newline='') as fp:
        for row in csv.reader(fp):
            row[0] = row[0].split('/')[-1]                                             # :97
            row[0] = row[0].split('.')[0]                                              # :98
            rows.append(row)
    return rows


def horizon_truth(metadata, image_file):
    """benchmark.py:205-220: the horizon through the two end points of the image's row (columns 3..6, in units the row's
    own height and width scale), or None for an image without a row."""
    base = image_file.split('/')[-1].split('.')[0]                                     # :207-208
    for row in metadata:
        if row[0] == base:
            width, height = float(row[2]), float(row[1])                              # :212-213
            scale = np.maximum(width, height)
            p1 = np.array([float(row[3]), float(row[4]), 1])
            p2 = np.array([float(row[5]), float(row[6]), 1])
            p1[0:2] /= scale / 2.0                                                     # :217-218
            p2[0:2] /= scale / 2.0
            return np.cross(p1, p2)                                                    # :219
    return None


def image_size(image_file):
    """(width, height) of an image file from its header, without decoding it."""
    from PIL import Image
    with Image.open(image_file) as im:
        return im.size


def load_ground_truth(dataset, dataset_name, source_folder):
    """Fills dataset['true_horizon'], dataset['true_vps'] and dataset['image_shape'] ((height, width) of the image FILE,
    which the reference reads at :123-126), one entry per dataset['image_files'].  dataset_name: "york", "eurasian" or
    "horizon".  An image whose file is missing gets None three times and no error (:119-121); an HLW image without a
    metadata row gets its shape and None for the rest (:247 leaves it out of the errors).  Returns the dataset."""
    if dataset_name not in ("york", "eurasian", "horizon"):
        raise ValueError("load_ground_truth: dataset_name must be york, eurasian or horizon, got %r" % (dataset_name,))
    if dataset_name == "york":
        K, S = york_camera(source_folder)
    elif dataset_name == "horizon":
        metadata = horizon_metadata(source_folder)
    horizons, vps, shapes = [], [], []
    for image_file in dataset['image_files']:
        if not os.path.isfile(image_file):
            horizons.append(None), vps.append(None), shapes.append(None)
            continue
        width, height = image_size(image_file)
        tv, th = None, None
        if dataset_name == "york":
            tv, th = york_truth(image_file, K, S)
        elif dataset_name == "eurasian":
            tv, th = eurasian_truth(image_file, width, height)
        else:
            th = horizon_truth(metadata, image_file)
        horizons.append(th), vps.append(tv), shapes.append((int(height), int(width)))
    dataset['true_horizon'], dataset['true_vps'], dataset['image_shape'] = horizons, vps, shapes
    return dataset
