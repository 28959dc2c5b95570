"""Front end of the pipeline: image -> grey levels -> line segments in normalised image
coordinates -> homogeneous lines -> sphere raster.  Mirrors evaluation.py:121-251 of the reference.

What can be pinned is pinned: `detect_lsd_lines` (the pixel -> normalised-coordinate arithmetic around the detector)
and the homogeneous lines of `create_data_dict_single` are checked against the reference's own functions run on known
detector output (tests/golden/frontend.npz, tests/test_frontend.py).  What cannot: the detector itself (lsd.py; the
reference's is an absent submodule), skimage's rgb2gray (absent here; its documented weights are used) and
ImageMagick's `convert -resize` (an external program in the reference, evaluation.py:142-143; Pillow's Lanczos
resampling stands in).  The raster comes from the GPU rasteriser like everywhere else in this package."""
import numpy as np

from . import lsd

_GRAY = np.array([0.2125, 0.7154, 0.0721])     # skimage.color.rgb2gray (evaluation.py:150,190)


def rgb2gray(image_rgb):
    """float64 luminance in [0, 1] for uint8 input, like skimage.color.rgb2gray."""
    a = np.asarray(image_rgb)
    if a.ndim == 2:
        return a.astype(np.float64) / (255.0 if a.dtype == np.uint8 else 1.0)
    f = a[..., :3].astype(np.float64)
    if a.dtype == np.uint8:
        f /= 255.0
    return f.dot(_GRAY)


def imread(path):
    """scipy.ndimage.imread (evaluation.py:145,148): the file as an array, RGB for colour images."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB"):
            im = im.convert("RGB")
        return np.asarray(im).copy()


def fit_size(w, h, target_size):
    """The (width, height) resize_to_fit scales a w x h image to: inside S x S, keeping the aspect ratio."""
    s = min(float(target_size) / w, float(target_size) / h)
    return max(1, int(np.floor(w * s + 0.5))), max(1, int(np.floor(h * s + 0.5)))


def resize_to_fit(image, target_size):
    """`convert file -resize SxS` (evaluation.py:142-143): scale to fit inside S x S keeping the aspect ratio."""
    from PIL import Image
    h, w = image.shape[:2]
    nw, nh = fit_size(w, h, target_size)
    im = Image.fromarray(image)
    return np.asarray(im.resize((nw, nh), Image.LANCZOS)).copy()


def detect_lsd_lines(image, detector=None):
    """evaluation.py:227-251: grey image -> {'segments': N x 4 in normalised coordinates, 'nfa': N}.
    x, y are centred, divided by half of the LONG side and y points up."""
    image = np.asarray(image).astype('float64')
    if np.max(image) <= 1:
        image = image * 255
    width = image.shape[1]
    height = image.shape[0]
    scale_w = np.maximum(width, height)
    scale_h = scale_w
    lsd_lines = np.array((detector or lsd.detect_line_segments)(image), dtype=np.float64)
    lsd_lines = lsd_lines.reshape(-1, 7)
    lsd_lines[:, 0] -= width / 2.0
    lsd_lines[:, 1] -= height / 2.0
    lsd_lines[:, 2] -= width / 2.0
    lsd_lines[:, 3] -= height / 2.0
    lsd_lines[:, 0] /= (scale_w / 2.0)
    lsd_lines[:, 1] /= (scale_h / 2.0)
    lsd_lines[:, 2] /= (scale_w / 2.0)
    lsd_lines[:, 3] /= (scale_h / 2.0)
    lsd_lines[:, 1] *= -1
    lsd_lines[:, 3] *= -1
    return {'segments': lsd_lines[:, 0:4], 'nfa': lsd_lines[:, 6]}


def homogeneous_lines(line_segments):
    """evaluation.py:161-168 / :199-208: l = cross((x1, y1, 1), (x2, y2, 1)) per segment."""
    seg = np.asarray(line_segments, dtype=np.float64).reshape(-1, 4)
    p1 = np.concatenate([seg[:, 0:2], np.ones((seg.shape[0], 1))], 1)
    p2 = np.concatenate([seg[:, 2:4], np.ones((seg.shape[0], 1))], 1)
    return np.cross(p1, p2)


def create_data_dict_single(image_rgb, cnn_input_size=250, detector=None, sphere_fn=None):
    """evaluation.py:188-224: one image -> {'lines': {...}, 'sphere_image': raster}."""
    image = rgb2gray(image_rgb)
    datum = {"image_shape": image.shape, "image": image_rgb}
    lsd_result = detect_lsd_lines(image, detector)
    datum['line_segments'] = lsd_result['segments']
    datum['lines'] = homogeneous_lines(lsd_result['segments'])
    if sphere_fn is None:
        from .evaluation import get_sphere_image as sphere_fn
    return {'lines': datum, 'sphere_image': sphere_fn(datum['lines'], size=cnn_input_size, alpha=0.1)}


def line_detector(image_file, target_size=None):
    """The callable evaluation.create_data_pickles plugs in: (image_file, target_size) -> (image_rgb, segments)."""
    image_rgb = imread(image_file)
    if target_size is not None:
        image_rgb = resize_to_fit(image_rgb, target_size)
    return image_rgb, detect_lsd_lines(rgb2gray(image_rgb))['segments']


def _detector_input(grey):
    """The image detect_lsd_lines hands to its detector."""
    image = np.asarray(grey).astype('float64')
    return image * 255 if np.max(image) <= 1 else image


def line_detector_batch(image_files, target_size=None, device=0):
    """line_detector for many files with ONE GPU detector call (lsd.detect_line_segments_batch): reading, resizing and
    grey conversion stay on the host.  -> the list of (image_rgb, segments) pairs line_detector would return."""
    rgbs = []
    for f in image_files:
        image_rgb = imread(f)
        if target_size is not None:
            image_rgb = resize_to_fit(image_rgb, target_size)
        rgbs.append(image_rgb)
    greys = [rgb2gray(im) for im in rgbs]
    raw = lsd.detect_line_segments_batch([_detector_input(g) for g in greys], device=device)
    return [(im, detect_lsd_lines(g, detector=lambda image, r=r: r)['segments']) for im, g, r in zip(rgbs, greys, raw)]


_DEVICE_CAP = 4096          # detector rows per image of lines_batch_device's first detector call
_DEVICE_MAX_PIXELS = 1 << 28       # 2 GiB of grey levels; fewer chunks keep the detector's one-wave-per-image region stage full


def lines_batch_device(images, target_size=None, device=0, cnn_input_size=None, keep_resized=False,
                       max_pixels=_DEVICE_MAX_PIXELS):
    """The front end for decoded images on GPU `device`, from uint8 pixels to the lines the raster and the EM read:
    fit-resize (resize_to_fit's Pillow Lanczos, byte for byte) and grey levels (vpk_image_prepare_batch), the detector
    (vpk_lsd_detect_batch, detected again with a larger buffer when an image overflows it), normalised segments and
    homogeneous lines (vpk_lsd_rows_to_lines, detect_lsd_lines + homogeneous_lines byte for byte) and, with
    ``cnn_input_size``, the sphere rasters (vpk_sphere_raster).  The images are uploaded once; only the segment counts
    come back to the host.  Grey levels are rgb2gray's to within a few ulp (include/vpk.h).
    images: uint8 arrays, H x W x 3 or H x W.  Works in chunks of at most ``max_pixels`` detector pixels (at least one
    image each); the results do not depend on the chunking.  Returns a dict keyed like em.upload_batch:
      offsets      host int64 (B+1) prefix sums of the line counts
      l, lp, nfa   device fp64 (sum N x 3, sum N x 4, sum N): homogeneous lines (pristine), segments, -log10(NFA)
      sphere       device uint8 (B x S x S) with cnn_input_size = S
      image_shape  (height, width) of each detector image
      images       with keep_resized: the resized uint8 images (host), as resize_to_fit returns them"""
    import ctypes
    from ._lib import VpkError
    from .runtime import get_runtime
    from .sphere_mapping import raster_batch_device, raster_flags
    imgs = [np.ascontiguousarray(im) for im in images]
    for im in imgs:
        if im.dtype != np.uint8 or not (im.ndim == 2 or (im.ndim == 3 and im.shape[2] == 3)):
            raise ValueError("lines_batch_device expects uint8 images of shape H x W x 3 or H x W")
    rt = get_runtime(device)
    torch = rt.torch
    dims = np.zeros((len(imgs), 5), dtype=np.int32)
    for k, im in enumerate(imgs):
        h, w = im.shape[:2]
        ow, oh = (w, h) if target_size is None else fit_size(w, h, target_size)
        dims[k] = (w, h, 1 if im.ndim == 2 else 3, ow, oh)
    px = dims[:, 3].astype(np.int64) * dims[:, 4]
    chunks, s = [], 0
    while s < len(imgs):
        e, tot = s + 1, px[s]
        while e < len(imgs) and tot + px[e] <= max_pixels:
            tot += px[e]
            e += 1
        chunks.append((s, e))
        s = e
    ptr = rt.ptr
    parts = []
    for s, e in chunks:
        d = np.ascontiguousarray(dims[s:e])
        n = e - s
        in_off = np.zeros(n + 1, dtype=np.int64)
        in_off[1:] = np.cumsum([imgs[k].size for k in range(s, e)])
        out_off = np.zeros(n + 1, dtype=np.int64)
        out_off[1:] = np.cumsum(px[s:e])
        det = np.ascontiguousarray(d[:, 3:5])
        with rt.on_stream():
            flat = torch.from_numpy(np.concatenate([imgs[k].ravel() for k in range(s, e)])).to(rt.tdev)
            grey = torch.empty(int(out_off[-1]), dtype=torch.float64, device=rt.tdev)
            resized = torch.empty(int((px[s:e] * d[:, 2]).sum()), dtype=torch.uint8, device=rt.tdev) if keep_resized else None
            rt.check(rt.lib.vpk_image_prepare_batch(rt.h, n, d.ctypes.data_as(ctypes.c_void_p),
                                                    in_off.ctypes.data_as(ctypes.c_void_p), ptr(flat),
                                                    out_off.ctypes.data_as(ctypes.c_void_p), ptr(resized), ptr(grey)))

            def detect(idx, cap):
                sub_off = np.zeros(len(idx) + 1, dtype=np.int64)
                sub_off[1:] = np.cumsum(px[s:e][idx])
                sub = grey if len(idx) == n else torch.cat([grey[out_off[i]:out_off[i + 1]] for i in idx])
                sd = np.ascontiguousarray(det[idx])
                rows = torch.empty((len(idx), cap, 7), dtype=torch.float64, device=rt.tdev)
                cnt = torch.empty(len(idx), dtype=torch.int32, device=rt.tdev)
                rt.check(rt.lib.vpk_lsd_detect_batch(rt.h, len(idx), sd.ctypes.data_as(ctypes.c_void_p),
                                                     sub_off.ctypes.data_as(ctypes.c_void_p), ptr(sub), 0.8, ptr(rows),
                                                     cap, ptr(cnt)))
                return rows, cnt.cpu().numpy()              # the one read: B counts (waits for the stream)

            cap = _DEVICE_CAP
            rows, counts = detect(np.arange(n), cap)
            again = np.nonzero(counts > cap)[0]
            if again.size:                                   # the detector's overflow rule: detect those again
                big = int(counts.max())
                more, c2 = detect(again, big)
                grown = torch.zeros((n, big, 7), dtype=torch.float64, device=rt.tdev)
                grown[:, :cap] = rows
                grown[torch.from_numpy(again).to(rt.tdev)] = more
                rows, cap = grown, big
                counts[again] = c2
            offs = np.zeros(n + 1, dtype=np.int64)
            offs[1:] = np.cumsum(counts)
            total = int(offs[-1])
            l = torch.empty((total, 3), dtype=torch.float64, device=rt.tdev)
            lp = torch.empty((total, 4), dtype=torch.float64, device=rt.tdev)
            nfa = torch.empty(total, dtype=torch.float64, device=rt.tdev)
            rt.check(rt.lib.vpk_lsd_rows_to_lines(rt.h, n, det.ctypes.data_as(ctypes.c_void_p), ptr(rows), cap,
                                                  offs.ctypes.data_as(ctypes.c_void_p), ptr(lp), ptr(l), ptr(nfa)))
        part = {"offsets": offs, "l": l, "lp": lp, "nfa": nfa, "resized": resized}
        if cnn_input_size is not None:
            part["sphere"] = raster_batch_device(rt, l if total else None, offs, int(cnn_input_size), 0.1)
            flags = raster_flags(rt, n)
            if flags.any():
                raise VpkError("sphere raster: the kernel's buffers were too small for a line of image(s) %s"
                                   % (np.nonzero(flags)[0] + s).tolist())
        parts.append(part)
    offsets = np.zeros(len(imgs) + 1, dtype=np.int64)
    base = 0
    for (s, e), p in zip(chunks, parts):
        offsets[s + 1:e + 1] = p["offsets"][1:] + base
        base += int(p["offsets"][-1])
    out = {"offsets": offsets, "image_shape": [(int(d[4]), int(d[3])) for d in dims]}
    with rt.on_stream():            # joined on the library's stream: ordered behind the chunks and before its next consumer
        cat = (lambda key: parts[0][key] if len(parts) == 1 else torch.cat([p[key] for p in parts]))
        if parts:
            out.update({"l": cat("l"), "lp": cat("lp"), "nfa": cat("nfa")})
            if cnn_input_size is not None:
                out["sphere"] = cat("sphere")
        else:
            out.update({k: torch.empty((0,) + sh, dtype=torch.float64, device=rt.tdev)
                        for k, sh in (("l", (3,)), ("lp", (4,)), ("nfa", ()))})
            if cnn_input_size is not None:
                out["sphere"] = torch.empty((0, int(cnn_input_size), int(cnn_input_size)), dtype=torch.uint8, device=rt.tdev)
    rt.synchronize()                # the results are complete for a consumer on any stream
    if keep_resized:
        res = []
        for (s, e), p in zip(chunks, parts):
            host = p["resized"].cpu().numpy()
            o = 0
            for k in range(s, e):
                w, h, ch = int(dims[k, 3]), int(dims[k, 4]), int(dims[k, 2])
                a = host[o:o + w * h * ch]
                res.append(a.reshape(h, w) if ch == 1 else a.reshape(h, w, 3))
                o += w * h * ch
        out["images"] = res
    return out


def line_detector_device(image_files, target_size=None, device=0):
    """line_detector for many files with the whole front end after decoding on the GPU (lines_batch_device): the
    list of (image_rgb, segments) pairs line_detector_batch returns."""
    rgbs = [imread(f) for f in image_files]
    r = lines_batch_device(rgbs, target_size, device=device, keep_resized=True)
    lp, offs = r["lp"].cpu().numpy(), r["offsets"]
    return [(im, lp[offs[k]:offs[k + 1]].copy()) for k, im in enumerate(r["images"])]
