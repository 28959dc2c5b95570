"""Times benchmark.py's two real-dataset flows on fabricated datasets (tests/test_gpu_benchmark_real.py: fabricate) on one
GPU: the 27-image YUD layout (640 x 480; the reference skips the first 25, so the pickle flow prepares and refines 27
images and scores 2, while the detector flow touches only the 2 it scores) and, for a like-for-like figure, a 27-image HLW
layout (start = 0: both flows handle all 27; 400 x 300 files resized to fit 800).  One warm-up, then the median of
``--runs`` runs per flow; decoding the image files (frontend.imread) is timed on its own.  The random-init net is built
once and shared by all runs (its weights take seconds to generate); no trained weights, so no accuracy is claimed.

    python scripts/time_benchmark_real.py [--runs 5]

Prints one JSON line per dataset and flow."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    args = p.parse_args()
    from test_gpu_benchmark_real import FLAG, fabricate
    from vanishing_points_2017_amd import benchmark, cnn, config, frontend
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    net = cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0), runtime=rt)
    benchmark.make_net = lambda device, cnn_range: net
    base = tempfile.mkdtemp(prefix="vp_bench_real_")
    config.cnn_weights_path = config.cnn_mean_path = os.path.join(base, "no_trained_weights")
    for name, attr in (("york", "yud_path"), ("horizon", "hlw_path")):
        root = fabricate(name, os.path.join(base, name), 27)
        setattr(config, attr, root)
        files = benchmark.real_dataset(name, os.path.join(base, "list"), True)[0]["image_files"]
        flows = {
            "pickles": [FLAG[name], "--result_dir", os.path.join(base, "pickles"), "--lsd", "gpu-frontend", "--update_datalist",
                        "--update_datafiles", "--run_cnn", "--run_em"],
            "detector": [FLAG[name], "--result_dir", os.path.join(base, "detector"), "--update_datalist", "--detector"],
        }
        decode = []
        for _ in range(args.runs + 1):
            t0 = time.perf_counter()
            for f in files:
                frontend.imread(f)
            decode.append(time.perf_counter() - t0)
        for flow, argv in flows.items():
            times, auc = [], None
            for _ in range(args.runs + 1):
                rt.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    auc = benchmark.main(argv)
                rt.synchronize()
                times.append(time.perf_counter() - t0)
            scored = 27 - (25 if name == "york" else 0)
            print(json.dumps({"dataset": name, "flow": flow, "images": 27, "scored": scored,
                              "images_processed": 27 if flow == "pickles" else scored, "runs": args.runs,
                              "median_s": statistics.median(times[1:]), "min_s": min(times[1:]), "max_s": max(times[1:]),
                              "warmup_s": times[0], "decode_all_27_files_median_s": statistics.median(decode[1:]), "auc": auc}),
                  flush=True)


if __name__ == "__main__":
    main()
