"""Benchmark driver with the reference's CLI (benchmark.py:16-26):

    python -m vanishing_points_2017_amd.benchmark --yud --result_dir /tmp/vp --update_datalist \\
        --update_datafiles --run_cnn --run_em [--lsd gpu-frontend] [--gpus N] [--save-overlays DIR]
    python -m vanishing_points_2017_amd.benchmark --yud --detector [--batch 64]
    python -m vanishing_points_2017_amd.benchmark --yud ... --synthetic [--count N]

Without --synthetic the images of the dataset's folder (config.yud_path / ecd_path / hlw_path, read when main runs) go
through the reference's flow (:39-75): get_data_list, create_data_pickles(cnn_input_size=500, target_size=800 for ECD and
HLW), run_cnn and run_em under their flags -- a random-init net stands in when no trained weights are configured, and a
line says so.  ground_truth.load_ground_truth reads the datasets' ground truth (:81-99, :137-220) and run_sharded scores:
horizon from the best orthogonal triplet, error = max end-point deviation / image height (:245-253), AUC up to 0.25
(:264).  The first 25 images of YUD and ECD are skipped (:69); an image whose file, pickle or metadata row is missing is
left out of the errors (:119-132, :247).

--detector is the pickle-free flow: the scored images are decoded on the host in chunks of --batch, every chunk goes
through detector.Detector.detect_device, its horizons and the uploaded ground truth through
calc_horizon.horizon_error_batch_device, and auc.calc_auc_device scores the concatenated errors; between the decode and
the AUC only the segment counts detect_device reads come back to the host.  The two flows order equal VP counts
differently, so they need not agree in every error.

``--synthetic`` replaces the dataset directory by the seeded synthetic set of the same shape (synth.CONFIGS): line
segments and ground-truth horizons come from the generator, rasters from the GPU rasteriser, and -- unless --run_cnn is
given together with real weight files -- the generator's response map stands in for a trained CNN's prediction."""
import argparse
import os
import time

import numpy as np

from . import auc as auc_mod, calc_horizon as ch, config, evaluation, sharding, sphere_mapping, synth

SHAPES = {"york": 2, "eurasian": 3, "horizon": 4}
ROOTS = {"york": "yud_path", "eurasian": "ecd_path", "horizon": "hlw_path"}      # config's attribute per dataset (:39-47)
EM_CONFIG = {'distance_measure': 'angle', 'use_weights': True, 'do_split': True, 'do_merge': True}     # :51


def build_parser():
    p = argparse.ArgumentParser(description='')
    p.add_argument('--yud', dest='yud', action='store_true', help='Run benchmark on YUD')
    p.add_argument('--ecd', dest='ecd', action='store_true', help='Run benchmark on ECD')
    p.add_argument('--hlw', dest='hlw', action='store_true', help='Run benchmark on HLW')
    p.add_argument('--result_dir', default='/tmp/', type=str, help='Directory to store (intermediate) results')
    p.add_argument('--gpu', default=0, type=int, help='GPU ID to use')
    p.add_argument('--update_datalist', dest='update_datalist', action='store_true', help='Update the dataset list')
    p.add_argument('--update_datafiles', dest='update_datafiles', action='store_true', help='Update the dataset files')
    p.add_argument('--run_cnn', dest='run_cnn', action='store_true', help='Evaluate CNN on the data')
    p.add_argument('--run_em', dest='run_em', action='store_true', help='Run EM refinement on the data')
    p.add_argument('--synthetic', action='store_true', help='use the seeded synthetic set of the dataset shape')
    p.add_argument('--count', type=int, default=None, help='number of synthetic images (default: dataset size)')
    p.add_argument('--force-dist', action='store_true',
                   help='initialise torch.distributed (RCCL unless VPK_DIST_BACKEND says otherwise) even with one rank: the N > 1 '
                        'code path -- process group, barriers, the record gather on the GPU -- on a one-GPU box')
    p.add_argument('--cnn-range', dest='cnn_range', choices=['raise', 'recompute_exact'], default='raise',
                   help='CNN range policy: raise on a clamped fp16-pair activation, or recompute those images exactly')
    p.add_argument('--gpus', type=int, default=1,
                   help='GPUs of this node to shard the images over (one process per GPU; results gathered with one '
                        'RCCL all_gather).  Without a launcher environment the ranks are started as child processes.')
    p.add_argument('--lsd', choices=['host', 'gpu', 'gpu-frontend'], default='host',
                   help='line segment detector of the real datasets: per image on the host, all images in one GPU batch, '
                        'or the whole front end after decoding (resize, grey, detector, lines, raster) on the GPU')
    p.add_argument('--detector', dest='detector', action='store_true',
                   help='real datasets without pickles: chunks of --batch images through detector.Detector, errors and AUC '
                        'on the GPU (not with --synthetic, not with --gpus > 1)')
    p.add_argument('--batch', type=int, default=64, help='images per chunk of --detector')
    p.add_argument('--save-overlays', dest='save_overlays', default=None, metavar='DIR',
                   help='real datasets: write one overlay per scored image to DIR (lines by vanishing point, the horizon; '
                        'the sphere panel marks the ground-truth VPs where the dataset has them)')
    return p


def target_size(name):
    """create_data_pickles' target_size at benchmark.py:59-60."""
    return 800 if name in ("eurasian", "horizon") else None


def real_dataset(name, result_dir, update):
    """benchmark.py:39-57: (the dataset dict of get_data_list for the dataset's folder, that folder)."""
    source = getattr(config, ROOTS[name])
    dest = os.path.join(result_dir, name)
    os.makedirs(dest, exist_ok=True)
    dataset = evaluation.get_data_list(source, dest, 'default_net', "", "0", update=update, dataset_name=name, **EM_CONFIG)
    return dataset, source


def subset(dataset, keep):
    """The dataset dict with its per-image lists cut down to the positions in ``keep``."""
    sub = dict(dataset)
    for k in ('image_files', 'pickle_files', 'true_horizon', 'true_vps', 'image_shape'):
        if k in dataset:
            sub[k] = [dataset[k][i] for i in keep]
    return sub


def scorable(dataset, start, need_pickles=True):
    """(positions the scoring keeps, how many of them lie before ``start``).  The reference's loop counts every image
    towards ``start`` (:113-115) and then leaves out an image whose file (:119-121) or pickle (:130-132) is missing or
    that has no ground truth (:247)."""
    keep = [i for i, f in enumerate(dataset['image_files'])
            if dataset['true_horizon'][i] is not None and os.path.isfile(f)
            and (not need_pickles or os.path.isfile(dataset['pickle_files'][i]))]
    return keep, sum(1 for i in keep if i < start)


def make_net(device, cnn_range):
    """The trained net of config's files, or -- as example.py does -- the random-init net and a line that says so."""
    from . import cnn
    if all(os.path.isfile(f) for f in (config.cnn_weights_path, config.cnn_mean_path)):
        return evaluation.init_caffe(config.cnn_config_path, config.cnn_weights_path, device, mean_file=config.cnn_mean_path,
                                     range_policy=cnn_range)._net
    print("no trained weights at %s: random-init AlexNet-500" % config.cnn_weights_path)
    net = cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0), device=device)
    net.set_range_policy(cnn_range)
    return net


def prepare_pickles(args, name, dataset, device):
    """benchmark.py:59-63 on the images whose files exist: create_data_pickles, and run_cnn under its flag."""
    present = subset(dataset, [i for i, f in enumerate(dataset['image_files']) if os.path.isfile(f)])
    evaluation.create_data_pickles(present, update=args.update_datafiles, cnn_input_size=500, target_size=target_size(name),
                                   lsd_device=device if args.lsd == 'gpu' else None,
                                   frontend_device=device if args.lsd == 'gpu-frontend' else None)
    if args.run_cnn:
        evaluation.run_cnn(present, None, None, None, gpu=device, net=make_net(device, args.cnn_range),
                           range_policy=args.cnn_range)


def save_overlays(directory, image_files, datums, images, horizons, true_vps, device=0):
    """--save-overlays: <name>_overlay.png per image (result_plotting's image panel: lines by VP and the horizon) and,
    where the datum has a sphere image, <name>_sphere.png with the ground-truth VPs marked after the result's."""
    from PIL import Image
    from . import result_plotting
    os.makedirs(directory, exist_ok=True)
    panels = result_plotting.render_em_results_batch(datums, images, true_vps=true_vps, horizons=horizons, device=device)
    out = []
    for f, p in zip(image_files, panels):
        base = os.path.join(directory, os.path.splitext(os.path.basename(f))[0])
        Image.fromarray(p['image']).save(base + "_overlay.png")
        if p['sphere'] is not None:
            Image.fromarray(p['sphere']).save(base + "_sphere.png")
        out.append(base + "_overlay.png")
    return out


def pickle_overlays(directory, dataset, start, device=0):
    """Overlays of the images run_sharded scored, from their pickles."""
    keep = list(range(start, len(dataset['pickle_files'])))
    datums = [evaluation._load_pickle(dataset['pickle_files'][i]) for i in keep]
    results = [d['EM_result'] if d['EM_result'] is not None and d['EM_result']['vp'] is not None
               else {'vp': np.zeros((0, 3)), 'counts': np.zeros(0)} for d in datums]
    hz = ch.calculate_horizon_batch(results, maxbest=20, theta_vmin=np.pi / 10, device=device) if results else []
    for d in datums:
        if d['EM_result'] is not None and d['EM_result']['vp'] is None:
            d['EM_result'] = None
    return save_overlays(directory, [dataset['image_files'][i] for i in keep], datums, [d['lines']['image'] for d in datums],
                         [((h[0][0], h[0][1]), (h[1][0], h[1][1])) for h in hz], [dataset['true_vps'][i] for i in keep], device)


def run_detector(args, name):
    """--detector: the scored images of a real dataset through detector.Detector in chunks of args.batch, horizon errors
    and AUC on the device.  Returns {'auc', 'errors' (device tensor, one per scored image), 'sorted_errors' (device),
    'image_files'}; the AUC is None when no image is left to score."""
    from . import frontend, ground_truth
    from .detector import Detector
    from .runtime import get_runtime
    if args.batch < 1:
        raise ValueError("--batch must be >= 1")
    device = args.gpu
    dataset, source = real_dataset(name, args.result_dir, args.update_datalist)
    ground_truth.load_ground_truth(dataset, name, source)
    start = 25 if name in ("york", "eurasian") else 0                         # :69
    keep = [i for i in scorable(dataset, start, need_pickles=False)[0] if i >= start]
    net = make_net(device, args.cnn_range)
    det = Detector(net, device=device, target_size=target_size(name), cnn_input_size=500, maxbest=20, theta_vmin=np.pi / 10.,
                   range_policy=args.cnn_range, **EM_CONFIG)
    rt = get_runtime(device)
    torch = rt.torch
    errors, t_decode, t0 = [], 0.0, time.time()
    for lo in range(0, len(keep), args.batch):
        chunk = keep[lo:lo + args.batch]
        t1 = time.time()
        images = [frontend.imread(dataset['image_files'][i]) for i in chunk]
        t_decode += time.time() - t1
        d = det.detect_device(images)
        with rt.on_stream():
            truth = torch.from_numpy(np.stack([np.asarray(dataset['true_horizon'][i], dtype=np.float64) for i in chunk])).to(rt.tdev)
        dims = [(dataset['image_shape'][i][1], dataset['image_shape'][i][0]) for i in chunk]     # of the image FILE (:125-126)
        errors.append(ch.horizon_error_batch_device(rt, d["horizon"], truth, dims))
        if args.save_overlays:
            host = det.host_results(d)
            shown = [im if target_size(name) is None else frontend.resize_to_fit(im, target_size(name)) for im in images]
            save_overlays(args.save_overlays, [dataset['image_files'][i] for i in chunk],
                          [{'lines': r['lines'], 'EM_result': r['EM_result']} for r in host], shown,
                          [((r['horizon'][0][0], r['horizon'][0][1]), (r['horizon'][1][0], r['horizon'][1][1])) for r in host],
                          [dataset['true_vps'][i] for i in chunk], device)
    res = {'auc': None, 'errors': None, 'sorted_errors': None, 'image_files': [dataset['image_files'][i] for i in keep]}
    if errors:
        with rt.on_stream():
            res['errors'] = torch.cat(errors)
        res['auc'], res['sorted_errors'] = auc_mod.calc_auc_device(rt, res['errors'], cutoff=0.25)
    res['seconds'], res['decode_seconds'] = time.time() - t0, t_decode
    return res


def synthetic_dataset(name, result_dir, count, update):
    """Writes reference-schema pickles for the synthetic set and returns the dataset dict."""
    cfg = SHAPES[name]
    dest = os.path.join(result_dir, name, "synthetic_angle_weights_split_merge")
    os.makedirs(dest, exist_ok=True)
    scenes = list(synth.config_scenes(cfg, count=count, raster=None))
    files = [os.path.join(dest, "img%05d.data.pkl" % i) for i in range(len(scenes))]
    dataset = {'source_folder': "synthetic:%s" % name, 'destination_folder': dest, 'use_weights': True,
               'distance_measure': "angle", 'do_split': True, 'do_merge': True, 'name': "synthetic_" + name,
               'image_files': ["synthetic:%s:%d" % (name, s["seed"]) for s in scenes], 'pickle_files': files,
               'true_horizon': [s["true_horizon"] for s in scenes], 'image_shape': [s["image_shape"] for s in scenes],
               'line_counts': [int(s["lp"].shape[0]) for s in scenes]}
    if update or not all(os.path.isfile(f) for f in files):
        rasters = sphere_mapping.raster_batch([s["l"] for s in scenes], size=500, alpha=0.1)
        for s, f, r in zip(scenes, files, rasters):
            datum = {"dataset": dataset["name"], "image_file": "synthetic", "image_shape": s["image_shape"],
                     "image": None, "line_segments": s["lp"], "lines": s["l"]}
            evaluation._dump_pickle({'lines': datum, 'sphere_image': r, 'cnn_prediction': s["cnn_response"]}, f)
    return dataset


def horizon_errors(dataset, indices, n_vp=20, theta_vmin=np.pi / 10, horizon_fn=None, device=0):
    """Per-image part of the scoring loop (benchmark.py:229-257) for the images in ``indices``: returns
    (em_results, errors).  ``horizon_fn`` defaults to the batched GPU selection."""
    todo = []
    for idx in indices:
        datum = evaluation._load_pickle(dataset['pickle_files'][int(idx)])
        em_result = datum.get('EM_result')
        assert em_result is not None, "no EM result!"                        # :231
        if em_result['vp'] is None:
            em_result = {'vp': np.zeros((0, 3)), 'counts': np.zeros(0)}
        todo.append(em_result)
    fn = horizon_fn or (lambda rs: ch.calculate_horizon_batch(rs, maxbest=n_vp, theta_vmin=theta_vmin, device=device))
    horizons = fn(todo) if todo else []
    errors = [ch.horizon_error(h[0], h[1], dataset['true_horizon'][int(idx)], dataset['image_shape'][int(idx)])
              for idx, h in zip(indices, horizons)]
    return todo, np.array(errors)


def run_sharded(dataset, rank=0, world=1, dist=None, device=0, start=0, run_em=True, em_fn=None,
                horizon_fn=None, err_cutoff=0.25, gather_on=None):
    """BASELINE configs[3]: the images of a dataset sharded over the ranks of one node.

    The reference's only multi-process facility is the start/end slice of run_em (evaluation.py:295-307).
    Here every rank (one process per GPU) takes one part of a cost-balanced partition (cost = N^2: the
    pairwise and smoothing work), refines and scores its images, and ONE all_gather of fixed-size records
    (sharding.pack_records / gather_records: RCCL over xGMI with the nccl backend, gloo on CPU) brings VPs,
    counts and horizon errors to every rank; rank 0 reports the AUC (benchmark.py:264).  No other exchange.
    ``em_fn(dataset, indices)`` defaults to evaluation.run_em on GPU ``device``; ``gather_on`` = torch device
    the records are gathered on (the rank's GPU for nccl, None = CPU tensors for gloo)."""
    n = len(dataset['pickle_files'])
    costs = np.asarray(dataset.get('line_counts', np.ones(n)), dtype=np.float64) ** 2
    mine = sharding.shard_balanced(costs, world)[rank]
    if run_em and len(mine):
        (em_fn or (lambda ds, idx: evaluation.run_em(ds, indices=idx, device=device)))(dataset, mine)
    results, errors = horizon_errors(dataset, mine, horizon_fn=horizon_fn, device=device)
    rec = sharding.pack_records(mine, results, errors)
    allrec = sharding.gather_records(dist, rec, device=gather_on) if dist is not None else rec
    assert allrec.shape[0] == n and np.array_equal(allrec[:, 0], np.arange(n)), "records lost in the gather"
    errs = allrec[start:, -1]
    auc, pts = auc_mod.calc_auc(errs.copy(), cutoff=err_cutoff)
    return auc, errs, allrec


def score(dataset, start=0, n_vp=20, theta_vmin=np.pi / 10, err_cutoff=0.25):
    """benchmark.py:108-266 with the ground truth supplied by the dataset dict."""
    errors = []
    todo = []
    for idx, data_file in enumerate(dataset['pickle_files']):
        if idx < start:
            continue
        datum = evaluation._load_pickle(data_file)
        em_result = datum.get('EM_result')
        assert em_result is not None, "no EM result!"                        # :231
        if em_result['vp'] is None:
            em_result = {'vp': np.zeros((0, 3)), 'counts': np.zeros(0)}
        todo.append((idx, em_result))
    # the reference calls calculate_horizon_and_ortho_vp image by image (:237-243); one batched launch here
    horizons = ch.calculate_horizon_batch([r for _, r in todo], maxbest=n_vp, theta_vmin=theta_vmin)
    for (idx, _), (hp1, hp2, _, _, _, _) in zip(todo, horizons):
        errors.append(ch.horizon_error(hp1, hp2, dataset['true_horizon'][idx], dataset['image_shape'][idx]))
    errors = np.array(errors)
    auc, pts = auc_mod.calc_auc(errors, cutoff=err_cutoff)
    return auc, errors, pts


def _spawn(args_list, gpus):
    """Start one process per GPU (torch.distributed.run) as children of this not-yet-GPU-initialised process."""
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "vanishing_points_2017_amd.benchmark"] + args_list
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def main(argv=None):
    import sys
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.detector and args.synthetic:
        parser.error("--detector runs on image files: it cannot be combined with --synthetic")
    if args.detector and args.gpus > 1:
        parser.error("--detector runs on one GPU: it cannot be combined with --gpus > 1 (sharding it is not implemented)")
    if args.yud:
        name = "york"
    elif args.ecd:
        name = "eurasian"
    elif args.hlw:
        name = "horizon"
    else:
        assert False                                                         # benchmark.py:49
    if args.detector:
        res = run_detector(args, name)
        print("decode + detector + scoring time (%d image(s), decoding %.3f s): " % (len(res['image_files']),
                                                                                      res['decode_seconds']), res['seconds'])
        print("AUC: ", res['auc'])
        return res['auc']
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return _spawn(list(sys.argv[1:] if argv is None else argv), args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    device = args.gpu
    backend = os.environ.get("VPK_DIST_BACKEND", "nccl")      # "gloo": ranks may share a GPU (tests on a one-GPU box)
    if world > 1 or args.force_dist:
        import torch
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29534")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        device = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(device)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group(backend=backend)
    start = 25 if (args.yud or args.ecd) else 0                              # :69
    if not args.synthetic:
        from . import ground_truth
        if rank == 0:    # one rank lists the images and writes their pickles; the others read them after the barrier
            dataset, source = real_dataset(name, args.result_dir, args.update_datalist)
            prepare_pickles(args, name, dataset, device)
        if dist is not None:
            dist.barrier()
        if rank != 0:
            dataset, source = real_dataset(name, args.result_dir, False)
        ground_truth.load_ground_truth(dataset, name, source)
        keep, start = scorable(dataset, start)
        if len(keep) <= start:
            raise ValueError("no image of %s is left to score: %d image(s) with a file, a pickle and ground truth, the "
                             "first %d skipped" % (source, len(keep), start))
        dataset = subset(dataset, keep)
        print("dataset name: ", dataset['name'])                             # :79
    if args.synthetic and rank == 0:    # one rank writes the input pickles; the others read them after the barrier
        dataset = synthetic_dataset(name, args.result_dir, args.count, args.update_datafiles or args.update_datalist)
    if dist is not None:
        dist.barrier()
    if args.synthetic and rank != 0:
        dataset = synthetic_dataset(name, args.result_dir, args.count, False)
    if args.synthetic and args.run_cnn and rank == 0:
        if not all(os.path.isfile(f) for f in (config.cnn_weights_path, config.cnn_mean_path)):
            print("no trained weights at %s: keeping the generator's response maps as cnn_prediction"
                  % config.cnn_weights_path)
        else:
            evaluation.run_cnn(dataset, mean_file=config.cnn_mean_path, model_def=config.cnn_config_path,
                               model_weights=config.cnn_weights_path, gpu=device, range_policy=args.cnn_range)
    if dist is not None:
        dist.barrier()
    t0 = time.time()
    tdev = None
    if dist is not None and backend == "nccl":
        import torch
        tdev = torch.device("cuda", device)
    auc, errors, _ = run_sharded(dataset, rank, world, dist, device=device, start=start, run_em=args.run_em,
                                 gather_on=tdev)
    if rank == 0:
        print("EM + scoring time (%d rank(s)%s): " % (world, "" if dist is None else ", records gathered over " + backend), time.time() - t0)
        print("AUC: ", auc)
        if args.save_overlays and not args.synthetic:
            pickle_overlays(args.save_overlays, dataset, start, device)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return auc


if __name__ == "__main__":
    main()
