"""The REFERENCE's ground-truth arithmetic on seeded fixtures -> tests/golden/ground_truth/ground_truth.npz.

TEST INFRASTRUCTURE, build container only (needs the reference tree -- VPK_REFERENCE_ROOT, as oracle/ref_shim.py finds it --
and SciPy).  The reference's benchmark.py is a Python 2 script that does everything at import, so it cannot be loaded.
This script reads its TEXT, cuts out

    :84-90     the York camera set-up (K, S)
    :96-99     the loop over metadata.csv's rows
    :137-220   scale and the three dataset branches
    :247-253   the error of a detected horizon

and compiles each piece in memory with Python 2's `/`: an ast transformer maps every Div (binary or augmented) to a helper
that floor-divides when both operands are Python or NumPy integers and divides truly otherwise.  The pieces run on the
fixtures below, read back through scipy.io.loadmat from .mat files this script writes to a temporary folder, and the file
stores inputs and outputs as arrays.  No reference text is stored.

    python scripts/make_ground_truth_golden.py

Keys (tests/test_ground_truth.py writes the same fixture files and holds ground_truth.py to the outputs bit for bit):
  yud_focal, yud_pixel_size, yud_pp        cameraParameters.mat;   yud_K, yud_S
  yud_vp (2 x 3 x 3)                       the `vp` matrices;      yud_true_vps (2 x 3 x 3), yud_true_horizon (2 x 3)
  ecd_size (4 x 2: width, height), ecd_zenith (4 x 1 x 2), ecd_hor_points (4 x 2 x 2), ecd_horizon (4 x 3),
  ecd_horizon_as_column (4, bool)          stored 3 x 1 instead of 1 x 3;   ecd_true_vps (4 x 3 x 3), ecd_true_horizon (4 x 3)
  ecd_floor_divisions (4)                  how many of the reference's divisions floored, per image
  hlw_rows (3 x 7 strings), hlw_files (4 strings: the last has no row)
  hlw_true_horizon (3 x 3), hlw_last_is_none
  detected (2 x 2: hP1[1], hP2[1])         two detected horizons, end points (1, y1, 1) and (-1, y2, 1)
  {yud,ecd,hlw}_errors (images x 2), {yud,ecd,hlw}_image_size (images x 2: width, height used for the error)"""
import ast
import copy
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from ref_shim import REFERENCE_ROOT  # noqa: E402
OUT = os.path.join(ROOT, "tests", "golden", "ground_truth", "ground_truth.npz")

FLOORED = [0]


def _is_int(x):
    if isinstance(x, bool):
        return False
    if isinstance(x, (int, np.integer)):
        return True
    return isinstance(x, np.ndarray) and np.issubdtype(x.dtype, np.integer)


def py2_div(a, b):
    """Python 2's `/` without `from __future__ import division`."""
    if _is_int(a) and _is_int(b):
        FLOORED[0] += 1
        return a // b
    return a / b


class Py2Division(ast.NodeTransformer):
    def _call(self, node, left, right):
        return ast.copy_location(ast.Call(func=ast.Name(id='_py2_div', ctx=ast.Load()), args=[left, right], keywords=[]), node)

    def visit_BinOp(self, node):
        self.generic_visit(node)
        return self._call(node, node.left, node.right) if isinstance(node.op, ast.Div) else node

    def visit_AugAssign(self, node):
        self.generic_visit(node)
        if not isinstance(node.op, ast.Div):
            return node
        load = copy.deepcopy(node.target)
        load.ctx = ast.Load()
        return ast.copy_location(ast.Assign(targets=[node.target], value=self._call(node, load, node.value)), node)


def piece(lines, first, last):
    """Lines first..last (1-based, inclusive) of the reference's benchmark.py, dedented and compiled with Python 2's `/`."""
    text = lines[first - 1:last]
    indent = min(len(ln) - len(ln.lstrip()) for ln in text if ln.strip())
    tree = Py2Division().visit(ast.parse("".join(ln[indent:] if ln.strip() else "\n" for ln in text)))
    ast.fix_missing_locations(tree)
    return compile(tree, "benchmark.py:%d-%d" % (first, last), "exec")


def run(code, **names):
    env = dict(names, np=np, _py2_div=py2_div)
    exec(code, env)
    return env


def main():
    from scipy import io
    with open(os.path.join(REFERENCE_ROOT, "benchmark.py")) as fp:
        lines = fp.readlines()
    camera, rows_loop, truth, error = piece(lines, 84, 90), piece(lines, 96, 99), piece(lines, 137, 220), piece(lines, 247, 253)
    rs = np.random.RandomState(20171)
    out = {}
    tmp = tempfile.mkdtemp()
    detected = np.array([[0.031, -0.044], [-0.35, 0.27]])
    out["detected"] = detected

    def errors(true_horizon, width, height):
        res = []
        for y1, y2 in detected:
            env = run(error, trueHorizon=None if true_horizon is None else np.array(true_horizon, dtype=np.float64),
                      hP1=np.array([1.0, y1, 1.0]), hP2=np.array([-1.0, y2, 1.0]), scale=np.maximum(width, height),
                      imageHeight=height)
            res.append(env["max_error"])
        return res

    # ---- YUD ----------------------------------------------------------------------------------------------------------
    out["yud_focal"], out["yud_pixel_size"], out["yud_pp"] = np.float64(6.0532), np.float64(0.0090), np.array([307.5513, 251.4542])
    cam_file = os.path.join(tmp, "cameraParameters.mat")
    io.savemat(cam_file, {"focal": out["yud_focal"], "pixelSize": out["yud_pixel_size"], "pp": out["yud_pp"]})
    env = run(camera, cameraParams=io.loadmat(cam_file))
    K, S = env["K"], env["S"]
    out["yud_K"], out["yud_S"] = np.asarray(K), np.asarray(S)
    vps, tvs, ths, errs = [], [], [], []
    for k in range(2):
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))                 # three orthogonal directions in columns
        q[:, 1] *= 1.0 + 0.2 * k                                    # the files do not promise unit length
        image_id = "P%07d" % (1020171 + k)
        os.makedirs(os.path.join(tmp, "yud", image_id))
        io.savemat(os.path.join(tmp, "yud", image_id, image_id + "GroundTruthVP_CamParams.mat"), {"vp": q})
        env = run(truth, dataset_name="york", io=io, K=K, S=S, path1=os.path.join(tmp, "yud"), imageID=image_id,
                  imageWidth=640, imageHeight=480)
        vps.append(q), tvs.append(np.asarray(env["trueVPs"])), ths.append(np.asarray(env["trueHorizon"]))
        errs.append(errors(ths[-1], 640, 480))
    out["yud_vp"], out["yud_true_vps"], out["yud_true_horizon"] = np.stack(vps), np.stack(tvs), np.stack(ths)
    out["yud_errors"], out["yud_image_size"] = np.array(errs), np.array([[640, 480]] * 2)

    # ---- ECD ----------------------------------------------------------------------------------------------------------
    sizes = [(321, 240), (320, 241), (323, 241), (239, 321)]       # odd width, odd height, both odd, both odd upright
    as_column = [False, True, False, True]
    zen, hor, hz, tvs, ths, errs, floored = [], [], [], [], [], [], []
    for k, ((w, h), col) in enumerate(zip(sizes, as_column)):
        zenith = np.array([[w / 2.0 + rs.uniform(-40, 40), -rs.uniform(800, 3000)]])
        hor_points = np.stack([[-rs.uniform(200, 900), h * rs.uniform(0.3, 0.6)], [w + rs.uniform(200, 900), h * rs.uniform(0.3, 0.6)]])
        horizon = np.cross(np.append(hor_points[0], 1.0), np.append(hor_points[1], 1.0))
        horizon /= np.linalg.norm(horizon[:2])
        base = os.path.join(tmp, "ecd%d" % k)
        io.savemat(base + "VP.mat", {"zenith": zenith, "hor_points": hor_points})
        io.savemat(base + "hor.mat", {"horizon": horizon.reshape(3, 1) if col else horizon.reshape(1, 3)})
        FLOORED[0] = 0
        env = run(truth, dataset_name="eurasian", io=io, basename=base, imageWidth=w, imageHeight=h)
        floored.append(FLOORED[0])
        zen.append(zenith), hor.append(hor_points), hz.append(horizon)
        tvs.append(np.asarray(env["trueVPs"])), ths.append(np.asarray(env["trueHorizon"]))
        errs.append(errors(ths[-1], w, h))
    assert floored == [3] * 4, floored                              # :180, :181, :183
    out.update(ecd_size=np.array(sizes), ecd_zenith=np.stack(zen), ecd_hor_points=np.stack(hor), ecd_horizon=np.stack(hz),
               ecd_horizon_as_column=np.array(as_column), ecd_true_vps=np.stack(tvs), ecd_true_horizon=np.stack(ths),
               ecd_floor_divisions=np.array(floored), ecd_errors=np.array(errs), ecd_image_size=np.array(sizes))

    # ---- HLW ----------------------------------------------------------------------------------------------------------
    rows = [["a1.jpg", "768", "1024", "-512.0", "35.25", "512.0", "-18.5"],
            ["flickr/b2.v1.jpg", "1200", "800", "-400.0", "-120.125", "400.0", "-96.75"],
            ["c3", "500", "500", "-250.0", "7.0", "250.0", "7.0"]]
    files = ["/data/HLW/images/a1.jpg", "/data/HLW/images/b2.jpg", "/data/HLW/images/c3.png", "/data/HLW/images/d4.jpg"]
    image_sizes = [(1024, 768), (533, 800), (500, 500), (640, 480)]
    env = run(rows_loop, metadata_file=[list(r) for r in rows], metadata=[])
    metadata = env["metadata"]
    ths, errs = [], []
    for f, (w, h) in zip(files, image_sizes):
        env = run(truth, dataset_name="horizon", image_file=f, metadata=metadata, imageWidth=w, imageHeight=h)
        assert env["trueVPs"] is None
        if env["trueHorizon"] is None:
            assert f == files[-1]
            continue
        ths.append(np.asarray(env["trueHorizon"])), errs.append(errors(ths[-1], w, h))
    assert len(ths) == 3
    out.update(hlw_rows=np.array(rows), hlw_files=np.array(files), hlw_true_horizon=np.stack(ths),
               hlw_last_is_none=np.array(True), hlw_errors=np.array(errs), hlw_image_size=np.array(image_sizes[:3]))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez(OUT, **out)
    shutil.rmtree(tmp)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    sys.exit(main())
