"""Single-image example with the reference's flags (example.py:11-14): --gpu, --show; --save-overlays DIR writes what the
reference's --show displays (example.py:82) as one image per input, headless (result_plotting.py).

With --source_folder DIR (the reference uses assets/examples, example.py:26) the images of DIR go through the
reference's three calls -- create_data_pickles(cnn_input_size=500, target_size=640), run_cnn, run_em (example.py:36-39)
-- with this package's front end (frontend.py), a random-init CNN unless trained weights are configured (config.py),
and the horizon end points are printed in pixel coordinates like example.py:66-76.  Without it one seeded synthetic
scene (configs[0]: N = 800) goes through raster, CNN and EM.  --detector sends the images of --source_folder through
detector.Detector instead: one GPU batch, the same printed lines, no pickles."""
import argparse

import numpy as np

from . import calc_horizon, cnn, evaluation, synth


def save_overlay(directory, name, panels):
    """One PNG per image under --save-overlays: the image panel (lines by VP, horizon)."""
    import os
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    out = os.path.join(directory, name + "_overlay.png")
    Image.fromarray(panels['image']).save(out)
    print("  overlay:", out)
    return out


def save_file_overlay(directory, image_file, datum, horizon_px=None, device=0):
    """--save-overlays for one image of --source_folder (example.py:82, to a file instead of a window): the image scaled
    to fit 640 like the front end's, its lines by VP and the horizon (pixel end points).  An image without vanishing
    points gets its plain (resized) image, so that every input has an overlay."""
    import os
    from . import result_plotting
    panels = result_plotting.show_em_result(datum, image_file, target_size=640, horizon=horizon_px, device=device)
    return save_overlay(directory, os.path.splitext(os.path.basename(image_file))[0], panels)


def run_folder(args):
    import os
    from . import config
    os.makedirs(args.destination_folder, exist_ok=True)
    dataset = evaluation.get_data_list(args.source_folder, args.destination_folder, 'default_net', "", "0",
                                       distance_measure='angle', use_weights=True, do_split=True, do_merge=True,
                                       update=True)                                   # example.py:30-34
    evaluation.create_data_pickles(dataset, update=True, cnn_input_size=500, target_size=640,       # :37
                                   lsd_device=args.gpu if args.lsd == 'gpu' else None,
                                   frontend_device=args.gpu if args.lsd == 'gpu-frontend' else None)
    if all(os.path.isfile(f) for f in (config.cnn_weights_path, config.cnn_mean_path)):
        evaluation.run_cnn(dataset, mean_file=config.cnn_mean_path, model_def=config.cnn_config_path,
                           model_weights=config.cnn_weights_path, gpu=args.gpu, range_policy=args.cnn_range)   # :38
    else:
        print("no trained weights at %s: random-init AlexNet-500" % config.cnn_weights_path)
        evaluation.run_cnn(dataset, None, None, None, gpu=args.gpu,
                           net=cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0), device=args.gpu),
                           range_policy=args.cnn_range)
    evaluation.run_em(dataset)                                                        # :39
    for image_file, data_file in zip(dataset['image_files'], dataset['pickle_files']):
        datum = evaluation._load_pickle(data_file)
        res = datum['EM_result']
        height, width = datum['lines']['image_shape'][:2]
        print(image_file, "%d x %d, %d line segments" % (width, height, datum['lines']['line_segments'].shape[0]))
        if res is None or res['vp'] is None:
            print("  no vanishing points")
            if args.save_overlays:
                save_file_overlay(args.save_overlays, image_file, datum, None, args.gpu)
            continue
        hp1, hp2, _, _, _, _ = calc_horizon.calculate_horizon_and_ortho_vp(res, maxbest=20, theta_vmin=np.pi / 10.)
        scale = max(width, height)
        for hp in (hp1, hp2):                                                          # :66-76
            hp[0] = hp[0] * scale / 2.0 + width / 2.0
            hp[1] = -hp[1] * scale / 2.0 + height / 2.0
        print("  VPs: %d, iterations: %d, horizon: (%.1f, %.1f) - (%.1f, %.1f)" % (
            res['vp'].shape[0], res['iterations'], hp1[0], hp1[1], hp2[0], hp2[1]))
        if args.save_overlays:
            save_file_overlay(args.save_overlays, image_file, datum, (hp1, hp2), args.gpu)
    return dataset


def run_folder_detector(args):
    """--detector: the images of --source_folder through detector.Detector.detect -- one batch on the GPU, no pickles --
    with run_folder's settings (cnn_input_size 500, target_size 640, maxbest 20) and its printed lines.  Returns detect's
    list, one result per image file."""
    import glob
    import os
    from . import config, frontend
    from .detector import Detector
    image_files = sorted(sum((glob.glob("%s/*.%s" % (args.source_folder, ext)) for ext in ("jpg", "png", "pgm")), []))
    if all(os.path.isfile(f) for f in (config.cnn_weights_path, config.cnn_mean_path)):
        net = evaluation.init_caffe(config.cnn_config_path, config.cnn_weights_path, args.gpu,
                                    mean_file=config.cnn_mean_path)._net
    else:
        print("no trained weights at %s: random-init AlexNet-500" % config.cnn_weights_path)
        net = cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0), device=args.gpu)
    det = Detector(net, device=args.gpu, target_size=640, cnn_input_size=500, maxbest=20, theta_vmin=np.pi / 10.,
                   range_policy=args.cnn_range, distance_measure='angle', use_weights=True, do_split=True, do_merge=True)
    results = det.detect([frontend.imread(f) for f in image_files])
    for image_file, r in zip(image_files, results):
        height, width = r['lines']['image_shape'][:2]
        print(image_file, "%d x %d, %d line segments" % (width, height, r['lines']['line_segments'].shape[0]))
        res = r['EM_result']
        datum = {'lines': r['lines'], 'EM_result': res}
        if res is None:
            print("  no vanishing points")
            if args.save_overlays:
                save_file_overlay(args.save_overlays, image_file, datum, None, args.gpu)
            continue
        hp1, hp2 = r['horizon_px']
        print("  VPs: %d, iterations: %d, horizon: (%.1f, %.1f) - (%.1f, %.1f)" % (
            res['vp'].shape[0], res['iterations'], hp1[0], hp1[1], hp2[0], hp2[1]))
        if args.save_overlays:
            save_file_overlay(args.save_overlays, image_file, datum, (hp1, hp2), args.gpu)
    return results


def main(argv=None):
    p = argparse.ArgumentParser(description='')
    p.add_argument('--gpu', default=0, type=int, help='GPU ID to use')
    p.add_argument('--show', dest='show', action='store_true', help='Show results (prints only)')
    p.add_argument('--save-overlays', dest='save_overlays', default=None, metavar='DIR',
                   help='write one overlay per image to DIR: lines coloured by vanishing point and the horizon')
    p.add_argument('--seed', default=1000, type=int)
    p.add_argument('--lines', default=800, type=int)
    p.add_argument('--source_folder', default=None, help='folder with images (jpg / png / pgm)')
    p.add_argument('--destination_folder', default='/tmp/vp_example_results')
    p.add_argument('--cnn-range', dest='cnn_range', choices=['raise', 'recompute_exact'], default='raise',
                   help='CNN range policy: raise on a clamped fp16-pair activation, or recompute those images exactly')
    p.add_argument('--lsd', choices=['host', 'gpu', 'gpu-frontend'], default='host',
                   help='line segment detector of --source_folder: per image on the host, all images in one GPU batch, '
                        'or the whole front end after decoding (resize, grey, detector, lines, raster) on the GPU')
    p.add_argument('--detector', dest='detector', action='store_true',
                   help='with --source_folder: all images through detector.Detector in one GPU batch, without pickles')
    args = p.parse_args(argv)
    if args.detector and not args.source_folder:
        p.error("--detector needs --source_folder")
    if args.source_folder:
        return run_folder_detector(args) if args.detector else run_folder(args)
    sc = synth.make_scene(args.seed, args.lines, 3, aspect_h=0.667, raster=None)
    datum = {'lines': {'lines': sc["l"], 'line_segments': sc["lp"], 'image_shape': sc["image_shape"]},
             'sphere_image': evaluation.get_sphere_image(sc["l"], size=500, alpha=0.1)}
    net = cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0), device=args.gpu)
    net.set_range_policy(args.cnn_range)
    datum['cnn_prediction'] = cnn.caffe_forward(net, datum['sphere_image'])
    print("CNN response (random-init weights): min %.3f max %.3f" % (datum['cnn_prediction'].min(),
                                                                     datum['cnn_prediction'].max()))
    datum['cnn_prediction'] = sc["cnn_response"]       # stand-in for a trained net's prediction
    datum = evaluation.run_em_single(datum)
    res = datum['EM_result']
    hp1, hp2, _, _, _, _ = calc_horizon.calculate_horizon_and_ortho_vp(res, maxbest=20, theta_vmin=np.pi / 10.)
    height, width = sc["image_shape"]
    horizon = ((hp1[0], hp1[1]), (hp2[0], hp2[1]))      # normalised, before the conversion below
    for hp in (hp1, hp2):
        hp[0] = hp[0] * 640 / 2.0 + width / 2.0
        hp[1] = -hp[1] * 640 / 2.0 + height / 2.0
    print(hp1)
    print(hp2)
    if args.save_overlays:                             # the synthetic scene has no photograph: its lines on black
        from . import result_plotting
        image = np.zeros((int(height), int(width), 3), dtype=np.uint8)
        panels = result_plotting.render_em_result(datum, image, horizon=horizon, device=args.gpu)
        save_overlay(args.save_overlays, "synthetic_seed%d" % args.seed, panels)
    print("VPs: %d, iterations: %d, inlier lines: %d / %d" % (res['vp'].shape[0], res['iterations'],
                                                           int((res['vp_assoc'] >= 0).sum()), args.lines))


if __name__ == "__main__":
    main()
