"""Decoded images -> vanishing points and horizons in pixel coordinates, in one call.

The reference's flow for a folder of images (example.py:30-76) is three passes over pickles -- create_data_pickles,
run_cnn, run_em -- then calculate_horizon_and_ortho_vp and a conversion to pixels per image.  `Detector` composes this
package's device entry points instead: frontend.lines_batch_device (resize, grey levels, line segments, lines, sphere
rasters), cnn.Net.forward_device, em.em_batch_device, calc_horizon.horizon_batch_device (the order of the best VPs from
vpk_vp_order_batch, then vpk_horizon_batch) and vpk_to_pixels_batch.  Between the upload of the images and the results
only the B segment counts the front end reads come back to the host."""
import ctypes

import numpy as np

from . import _lib, calc_horizon, em, frontend
from .runtime import get_runtime

VPK_EM_NO_VP = 1          # include/vpk.h: the reference's all-None result


def _check_images(images):
    """lines_batch_device's rule, applied before anything touches the GPU."""
    imgs = [np.asarray(im) for im in images]
    for im in imgs:
        if im.dtype != np.uint8 or not (im.ndim == 2 or (im.ndim == 3 and im.shape[2] == 3)):
            raise ValueError("Detector expects uint8 images of shape H x W x 3 or H x W")
    return imgs


class Detector(object):
    """net: a cnn.Net.  target_size: fit-resize the images inside S x S first (None: as they are).  maxbest, theta_vmin,
    theta_z: calculate_horizon_and_ortho_vp's (example.py:61 uses maxbest = 20).  range_policy: None (leave the net's as
    it is), "raise" or "recompute_exact", as pipeline.Step takes it.  em_keywords: expectation_maximisation's
    (vp_localisation.py:168-172), distance_measure "angle" or "dotprod" included; an unknown keyword or measure is refused
    here, before the GPU is touched."""

    def __init__(self, net, device=0, target_size=None, cnn_input_size=500, maxbest=20, theta_vmin=np.pi / 10.,
                 theta_z=np.pi / 4., range_policy=None, **em_keywords):
        self.distance_measure = em_keywords.get("distance_measure", "angle")
        em._measure(self.distance_measure)
        for k in ("init_vp", "sphere_image"):
            if k in em_keywords:
                raise TypeError("Detector: %r belongs to one image, not to a detector" % k)
        self.params = em._params(em_keywords)
        if not 1 <= int(maxbest) <= 64:
            raise ValueError("maxbest must be 1..64 (vpk_horizon_batch), got %r" % (maxbest,))
        if range_policy is not None:
            from .cnn import range_policy_code
            range_policy_code(range_policy)
        self.net, self.device, self.target_size = net, int(device), target_size
        self.cnn_input_size, self.maxbest = int(cnn_input_size), int(maxbest)
        self.theta_vmin, self.theta_z, self.range_policy = float(theta_vmin), float(theta_z), range_policy

    def _response(self, rt, sphere):
        """net.forward_device on the rasters, its value range checked as the policy says."""
        net = self.net
        if self.range_policy is not None:
            net.set_range_policy(self.range_policy)
        if int(sphere.shape[0]) == 0:
            return rt.torch.empty((0, 20, 20), dtype=rt.torch.float32, device=rt.tdev)
        resp = net.forward_device(sphere)
        net.check_range()                       # waits for the forward: VpkRangeError under "raise"
        if net.rt is not rt:
            rt.stream.wait_stream(net.rt.stream)
        return resp

    def _em(self, rt, fe, cnn, max_vp=em.MAX_VP):
        """em.em_batch_device on the images with three or more segments; the others get the reference's all-None result
        (with fewer than three lines no VP keeps counts >= 3, vp_localisation.py:250-260) without a launch.  Returns the
        EM's dict for the whole batch plus "l_norm", the lines as the EM normalised them (pristine where it did not run)."""
        torch = rt.torch
        offsets = fe["offsets"]
        batch, total = len(offsets) - 1, int(offsets[-1])
        n = np.diff(offsets)
        keep = np.nonzero(n >= 3)[0]
        with rt.on_stream():
            l_norm = fe["l"].clone()
            if batch and keep.size == batch:
                out = em.em_batch_device(rt, offsets, l_norm, fe["lp"], cnn, fe["sphere"], None, self.params, max_vp,
                                         distance_measure=self.distance_measure)
                out["l_norm"] = l_norm
                return out
            dev = rt.tdev
            z = lambda shape, dtype, fill=0: torch.full(shape, fill, dtype=dtype, device=dev)
            out = {"vp": z((batch, max_vp, 3), torch.float64), "sigma": z((batch, max_vp), torch.float64),
                   "counts": z((batch, max_vp), torch.float64), "counts_weighted": z((batch, max_vp), torch.float64),
                   "num_vp": z((batch,), torch.int32), "vp_assoc": z((max(total, 1),), torch.int64, -1),
                   "iterations": z((batch,), torch.int32), "status": z((batch,), torch.int32, VPK_EM_NO_VP),
                   "flags": z((batch,), torch.int32), "metric": None, "trace": None, "l_norm": l_norm}
            if keep.size:
                sub_off = np.zeros(keep.size + 1, dtype=np.int64)
                sub_off[1:] = np.cumsum(n[keep])
                rows = torch.from_numpy(np.concatenate([np.arange(offsets[b], offsets[b + 1]) for b in keep])).to(dev)
                idx = torch.from_numpy(keep).to(dev)
                l_sub = fe["l"].index_select(0, rows)
                sub = em.em_batch_device(rt, sub_off, l_sub, fe["lp"].index_select(0, rows),
                                         cnn.reshape(batch, 400).index_select(0, idx), fe["sphere"].index_select(0, idx),
                                         None, self.params, max_vp, distance_measure=self.distance_measure)
                for k in ("vp", "sigma", "counts", "counts_weighted", "num_vp", "iterations", "status", "flags"):
                    out[k].index_copy_(0, idx, sub[k])
                out["vp_assoc"].index_copy_(0, rows, sub["vp_assoc"][:int(sub_off[-1])])
                l_norm.index_copy_(0, rows, l_sub)
        return out

    def detect_device(self, images, cnn_response=None, on_stage=None):
        """images: a list of decoded uint8 arrays, H x W x 3 or H x W.  cnn_response: None to run the net on the sphere
        rasters, or B x 20 x 20 float32 response maps on the device for the EM to refine on instead (as pipeline.Step's
        em_prior).  Returns one dict of device tensors (offsets and image_shape on the host):
          offsets, l, lp, nfa, sphere, image_shape    frontend.lines_batch_device's
          cnn                                         the response maps the EM used
          vp, sigma, counts, counts_weighted, num_vp, vp_assoc, iterations, status, flags    em.em_batch_device's
          l_norm                                      the lines as the EM normalised them
          order, horizon (B x 15), combo              calc_horizon.horizon_batch_device's
          lp_px (sum N x 4), vp_px (B x max_vp x 2, NaN past num_vp), horizon_px (B x 2 x 2)    pixels of the detector image
        An image with fewer than three segments is not refined: num_vp 0, status VPK_EM_NO_VP and the no-VP default horizon
        (calc_horizon.py:212-217).  The results are complete on return for a consumer on any stream.
        on_stage: None, or a callable given the runtime and "start", "frontend", "cnn", "em", "horizon", "pixels" in turn, each
        once that stage is enqueued (scripts/time_detector.py records an event on the runtime's stream there)."""
        imgs = _check_images(images)
        rt = get_runtime(self.device)
        torch = rt.torch
        mark = (lambda name: on_stage(rt, name)) if on_stage is not None else (lambda name: None)
        mark("start")
        fe = frontend.lines_batch_device(imgs, self.target_size, device=self.device, cnn_input_size=self.cnn_input_size)
        mark("frontend")
        batch = len(imgs)
        if cnn_response is None:
            cnn = self._response(rt, fe["sphere"])
        else:
            cnn = cnn_response
            if tuple(cnn.shape) != (batch, 20, 20) or cnn.dtype != torch.float32 or not cnn.is_cuda:
                raise ValueError("cnn_response must be a float32 device tensor of shape (%d, 20, 20)" % batch)
            rt.stream.wait_stream(torch.cuda.current_stream(cnn.device))
        mark("cnn")
        res = {k: fe[k] for k in ("offsets", "l", "lp", "nfa", "sphere", "image_shape")}
        res["cnn"] = cnn
        res.update(self._em(rt, fe, cnn))
        mark("em")
        hz = calc_horizon.horizon_batch_device(rt, res["vp"], res["counts"], res["num_vp"], self.maxbest, self.theta_vmin,
                                               self.theta_z)
        res.update({"order": hz["order"], "horizon": hz["out"], "combo": hz["combo"]})
        mark("horizon")
        dims = np.ascontiguousarray([(w, h) for h, w in fe["image_shape"]], dtype=np.int32).reshape(batch, 2)
        offsets = _lib.host_i64(fe["offsets"])
        max_vp = int(res["vp"].shape[1])
        with rt.on_stream():
            res["lp_px"] = torch.empty_like(fe["lp"])
            res["vp_px"] = torch.empty((batch, max_vp, 2), dtype=torch.float64, device=rt.tdev)
            res["horizon_px"] = torch.empty((batch, 2, 2), dtype=torch.float64, device=rt.tdev)
            rt.check(rt.lib.vpk_to_pixels_batch(rt.h, batch, dims.ctypes.data_as(ctypes.c_void_p),
                                                offsets.ctypes.data_as(ctypes.c_void_p), rt.ptr(fe["lp"]), max_vp,
                                                rt.ptr(res["vp"]), rt.ptr(res["num_vp"]), rt.ptr(res["horizon"]),
                                                rt.ptr(res["lp_px"]), rt.ptr(res["vp_px"]), rt.ptr(res["horizon_px"])))
        mark("pixels")
        rt.synchronize()
        return res

    def detect(self, images):
        """detect_device with host output: one dict per image with
          EM_result         the reference's result dict (vp_localisation.py:441-442, as em.em_batch builds it), or None when
                            the EM returned no VPs (status 1) or found no initial VP (status 2)
          status            the EM's status (include/vpk.h: vpk_em_status)
          horizon           (hP1, hP2, zVP, hVP1, hVP2, best_combo) of calculate_horizon_and_ortho_vp
          horizon_px, vp_px, line_segments_px    2 x 2, M x 2 and N x 4 in pixels of the detector image
          lines             create_data_dict_single's `lines` datum without the image: image_shape, line_segments, lines
        Unlike evaluation.run_em_batch no exception is raised mid-batch for an image without an initial VP: the image gets
        EM_result None and its status says why."""
        return self.host_results(self.detect_device(images))

    @staticmethod
    def host_results(d):
        """detect's list from detect_device's dict."""
        offs = d["offsets"]
        keys = ("l", "lp", "vp", "sigma", "counts", "counts_weighted", "num_vp", "vp_assoc", "iterations", "status", "flags",
                "l_norm", "horizon", "combo", "lp_px", "vp_px", "horizon_px")
        host = {k: d[k].cpu().numpy() for k in keys}
        host["metric"] = None
        results = []
        for b in range(len(offs) - 1):
            lo, hi = int(offs[b]), int(offs[b + 1])
            m, status = int(host["num_vp"][b]), int(host["status"][b])
            o, c = host["horizon"][b], host["combo"][b]
            results.append({
                "EM_result": em.host_result(host, host["l_norm"], lo, hi, b) if status == 0 else None,
                "status": status,
                "horizon": (o[0:3].copy(), o[3:6].copy(), o[6:9].copy(), o[9:12].copy(), o[12:15].copy(),
                            c.astype(np.int64) if c[2] >= 0 else c[:2].astype(np.int64)),
                "horizon_px": host["horizon_px"][b].copy(), "vp_px": host["vp_px"][b, :m].copy(),
                "line_segments_px": host["lp_px"][lo:hi].copy(),
                "lines": {"image_shape": tuple(d["image_shape"][b]), "line_segments": host["lp"][lo:hi].copy(),
                          "lines": host["l"][lo:hi].copy()}})
        return results
