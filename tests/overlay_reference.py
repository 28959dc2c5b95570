"""The overlay renderer of DESIGN section 7d restated in NumPy float64 -- plain loops over the primitives, vectorised over
the pixels -- with an np.longdouble variant of the sub-sample test, and the cases both tiers run (tests/test_overlay.py:
the host build of csrc/overlay_device.hpp; tests/test_gpu_overlay.py: the kernels).

The rule the tests hold the device code to (``check``): every pixel equals the float64 reference, except pixels that own
a CLOSE sub-sample of some primitive -- one whose extended-precision squared distance d2 lies within
1e-9 * max(d2, (w/2)^2, 1e-300) of (w/2)^2, so that rounding alone decides its side.  For such a primitive the pixel's
coverage may be off by one sub-sample step, |delta a| <= 16; the bound is carried through the blend formula as an
interval per channel (the blend is monotone in a and in d, so its extremes lie at the interval ends).  At most 0.1 % of
the pixels a case draws may be close, and outside the close sub-samples the float64 and the longdouble test must agree;
both are asserted for every case."""
import functools

import numpy as np

CLOSE_REL = 1e-9
CLOSE_CAP = 1e-3
SUB = (np.arange(4) + 0.5) / 4          # 0.125, 0.375, 0.625, 0.875: exact


def _d2(px, py, qx, qy, sx, sy):
    """Squared distance from the points (sx, sy) to the closed segment pq in the dtype of the arguments: the arithmetic of
    line_segment_point_distance (the reference's vp_localisation.py:743-758) before its square root; a segment without
    length is its end point."""
    dx, dy = qx - px, qy - py
    nrm = np.sqrt(dx * dx + dy * dy)
    nn = nrm * nrm
    if not nn > 0:
        ex, ey = px - sx, py - sy
        return ex * ex + ey * ey
    t = ((sx - px) * dx + (sy - py) * dy) / nn
    cx = np.where(t < 0, px, np.where(t > 1, qx, px + t * dx))
    cy = np.where(t < 0, py, np.where(t > 1, qy, py + t * dy))
    ex, ey = cx - sx, cy - sy
    return ex * ex + ey * ey


def _blend(c, d, a):
    return (c * a + d * (255 - a) + 127) // 255


def render(image, geom, rgba, width, extended=True):
    """Blend the primitives, in order, into a copy of the uint8 H x W x 3 ``image``.  geom (P, 4) end points or (P, 2) disc
    centres; rgba (P, 4) uint8, opacity = A / 255; width (P,).  Returns a dict: 'rgb' the float64 result; 'lo' / 'hi'
    the per-channel interval a device result may lie in (equal to 'rgb' wherever no sub-sample is close); 'drawn' /
    'close' pixel masks; 'disagree' the number of sub-samples outside the close ones on which float64 and longdouble
    differ.  extended=False skips the longdouble pass (lo = hi = rgb)."""
    img = np.array(image, dtype=np.int64)
    H, W = img.shape[:2]
    lo, hi = img.copy(), img.copy()
    drawn, close_pix = np.zeros((H, W), bool), np.zeros((H, W), bool)
    disagree = 0
    geom = np.asarray(geom, dtype=np.float64)
    if geom.ndim == 2 and geom.shape[1] == 2:
        geom = np.concatenate([geom, geom], axis=1)
    geom = geom.reshape(-1, 4)
    L = np.longdouble
    for g, col, w in zip(geom, np.asarray(rgba, dtype=np.int64).reshape(-1, 4), np.asarray(width, dtype=np.float64).reshape(-1)):
        if not (np.isfinite(g).all() and np.isfinite(w) and w >= 0):
            continue
        hw = w / 2
        x_lo, x_hi = int(np.floor(min(g[0], g[2]) - hw)) - 1, int(np.ceil(max(g[0], g[2]) + hw)) + 1
        y_lo, y_hi = int(np.floor(min(g[1], g[3]) - hw)) - 1, int(np.ceil(max(g[1], g[3]) + hw)) + 1
        x_lo, x_hi, y_lo, y_hi = max(x_lo, 0), min(x_hi, W), max(y_lo, 0), min(y_hi, H)
        if x_lo >= x_hi or y_lo >= y_hi:
            continue
        ys, xs = np.mgrid[y_lo:y_hi, x_lo:x_hi]
        k = np.zeros(xs.shape, np.int64)
        kc = np.zeros(xs.shape, np.int64)
        rr = hw * hw
        for j in range(4):
            for i in range(4):
                sx, sy = xs + SUB[i], ys + SUB[j]
                inside = _d2(g[0], g[1], g[2], g[3], sx, sy) <= rr
                k += inside
                if extended:
                    d2l = _d2(L(g[0]), L(g[1]), L(g[2]), L(g[3]), sx.astype(L), sy.astype(L))
                    rrl = (L(w) / 2) * (L(w) / 2)
                    cl = np.abs(d2l - rrl) <= CLOSE_REL * np.maximum(np.maximum(d2l, rrl), L(1e-300))
                    kc += cl
                    disagree += int(((d2l <= rrl) != inside)[~cl].sum())
        opacity = float(col[3]) / 255.0
        a = np.floor(255.0 * (k / 16.0) * opacity + 0.5).astype(np.int64)
        a_lo = np.where(kc > 0, np.maximum(a - 16, 0), a)
        a_hi = np.where(kc > 0, np.minimum(a + 16, 255), a)
        sl = (slice(y_lo, y_hi), slice(x_lo, x_hi))
        for ch in range(3):
            c = int(col[ch])
            corners = [_blend(c, d, aa) for d in (lo[sl + (ch,)], hi[sl + (ch,)]) for aa in (a_lo, a_hi)]
            lo[sl + (ch,)] = np.minimum.reduce(corners)
            hi[sl + (ch,)] = np.maximum.reduce(corners)
            img[sl + (ch,)] = _blend(c, img[sl + (ch,)], a)
        drawn[sl] |= (k > 0) | (kc > 0)
        close_pix[sl] |= kc > 0
    return {'rgb': img.astype(np.uint8), 'lo': lo, 'hi': hi, 'drawn': drawn, 'close': close_pix, 'disagree': disagree}


def check(got, ref, exact=False):
    """The rule of the module docstring for one image; ``exact``: equal outright, close sub-samples or not."""
    assert got.dtype == np.uint8 and got.shape == ref['rgb'].shape
    assert ref['disagree'] == 0
    n_drawn, n_close = int(ref['drawn'].sum()), int(ref['close'].sum())
    if exact:
        assert np.array_equal(got, ref['rgb'])
        return
    assert n_close <= CLOSE_CAP * n_drawn, (n_close, n_drawn)
    far = ~ref['close']
    assert np.array_equal(got[far], ref['rgb'][far])
    g = got.astype(np.int64)
    assert ((ref['lo'] <= g) & (g <= ref['hi'])).all()


# ---- the cases ------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (16, 16), (17, 33), (40, 23))          # W x H: tiles full and ragged in both directions
COUNTS = (0, 1, 255, 256, 257)                          # the chunk edge


def background(rng, w, h):
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


def random_segments(rng, n, w, h):
    """n seeded segments around a w x h image: end points from a continuous distribution (never on the sub-sample
    lattice), widths 0.5 .. 4, any colour, opacity 1, 0.6 or seeded; every 17th has no length, every 23rd lies outside."""
    g = np.stack([rng.uniform(-4, w + 4, n), rng.uniform(-4, h + 4, n), rng.uniform(-4, w + 4, n), rng.uniform(-4, h + 4, n)], axis=1)
    g[16::17, 2:] = g[16::17, :2]
    g[22::23] += w + h + 20.0
    rgba = rng.randint(0, 256, (n, 4)).astype(np.uint8)
    rgba[0::3, 3] = 255
    rgba[1::3, 3] = 153
    return g.reshape(n, 4), rgba, rng.uniform(0.5, 4.0, n)


def random_discs(rng, n, s):
    """n seeded discs on an s x s panel, opacity 0.6, diameters 6 .. 20: they overlap each other and the panel's edge."""
    xy = rng.uniform(-3, s + 3, (n, 2))
    rgba = rng.randint(0, 256, (n, 4)).astype(np.uint8)
    rgba[:, 3] = 153
    return xy, rgba, rng.uniform(6.0, 20.0, n)


def _one(w, h, geom, rgba, width, seed=1):
    rng = np.random.RandomState(seed)
    return {'disc': False, 'images': [background(rng, w, h)],
            'prims': [(np.array(geom, dtype=np.float64).reshape(-1, 4), np.array(rgba, dtype=np.uint8).reshape(-1, 4),
                       np.array(width, dtype=np.float64).reshape(-1))]}


RED, BLUE = (255, 0, 0, 255), (0, 0, 255, 255)
CROSS = [[5.3, 11.2, 33.1, 12.9], [20.4, 2.2, 19.1, 21.7]]


@functools.lru_cache(maxsize=None)
def case(name):
    """One named case: {'disc', 'images': [uint8 H x W x 3], 'prims': [(geom, rgba, width)], 'exact'}.  Treat as read-only."""
    rng = np.random.RandomState(abs(hash_name(name)) % (2 ** 31))
    c = None
    if name.startswith("count"):                        # the four sizes in one launch, each with P seeded segments
        p = int(name[5:])
        c = {'disc': False, 'images': [background(rng, w, h) for w, h in SIZES],
             'prims': [random_segments(rng, p, w, h) for w, h in SIZES]}
    elif name == "outside":                             # wholly outside: nothing may change
        c = _one(40, 23, [[-30.0, -9.5, -6.2, -8.1], [45.3, 30.2, 60.1, 27.7]], [RED, BLUE], [2, 10])
    elif name == "bbox_only":                           # the box touches the tile at x < 16, y >= 16; the capsule does not
        c = _one(40, 23, [[10.3, 1.2, 30.4, 21.1]], [RED], [2])
    elif name == "zero_length":
        c = _one(40, 23, [[15.7, 16.2, 15.7, 16.2], [3.3, 3.1, 3.3, 3.1]], [RED, BLUE], [9.3, 0.9])
    elif name == "wide_four_tiles":                     # width 10 across the corner shared by four tiles
        c = _one(40, 23, [[12.2, 12.4, 20.3, 19.8]], [(10, 200, 90, 255)], [10])
    elif name == "order_ab":
        c = _one(40, 23, CROSS, [RED, BLUE], [3, 3])
    elif name == "order_ba":
        c = _one(40, 23, CROSS[::-1], [BLUE, RED], [3, 3])
    elif name == "discs":                               # opacity 0.6, over each other and over the edge
        sizes = (17, 40)
        c = {'disc': True, 'images': [background(rng, s, s) for s in sizes], 'prims': [random_discs(rng, 12, s) for s in sizes]}
    elif name == "ragged":                              # [0, 1, 257] primitives on three sizes in one launch
        dims = ((17, 33), (1, 1), (40, 23))
        c = {'disc': False, 'images': [background(rng, w, h) for w, h in dims],
             'prims': [random_segments(rng, p, w, h) for p, (w, h) in zip((0, 1, 257), dims)]}
    elif name == "lattice":
        # horizontal and vertical segments on pixel boundaries and on the sub-sample lattice, widths 2 and 10: sub-samples
        # lie at distance exactly w / 2 from the segment's side and from its caps (the <= rule on representable values)
        c = _one(40, 23, [[4.125, 8.125, 20.125, 8.125], [30.375, 2.625, 30.375, 18.625], [4.0, 16.0, 36.0, 16.0],
                          [8.0, 1.0, 8.0, 22.0], [2.125, 11.375, 37.875, 11.375], [22.625, 5.875, 22.625, 14.125]],
                 [RED, BLUE, (0, 255, 0, 255), (255, 255, 0, 153), (0, 255, 255, 255), (255, 0, 255, 153)], [2, 2, 2, 2, 10, 10])
        c['exact'] = True
    assert c is not None, name
    c.setdefault('exact', False)
    return c


def hash_name(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) * 7919


CASES = tuple("count%d" % p for p in COUNTS) + ("outside", "bbox_only", "zero_length", "wide_four_tiles", "order_ab", "order_ba",
                                                "discs", "ragged", "lattice")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference results of a case, one per image; computed once and shared.  Treat as read-only."""
    c = case(name)
    return tuple(render(im, *pr) for im, pr in zip(c['images'], c['prims']))


GOLDEN_SCENES = ("yud_n120", "tiny_n12", "ecd_n300_v8")      # stored EM results of the reference, three different N


@functools.lru_cache(maxsize=None)
def golden_datum(name, w=64, h=48):
    """A stored scene as the datum run_em writes, a seeded w x h RGB image for it, its true VPs and its horizon (two
    normalised end points).  Treat as read-only."""
    from golden_util import load
    g = load(name)
    datum = {'lines': {'lines': g['l'], 'line_segments': g['lp']}, 'sphere_image': g['sphere_image'],
             'cnn_prediction': g['cnn_response'],
             'EM_result': {'vp': g['o_vp'], 'counts': g['o_counts'], 'vp_assoc': g['o_vp_assoc']}}
    horizon = ((g['h_hP1'][0], g['h_hP1'][1]), (g['h_hP2'][0], g['h_hP2'][1]))
    return datum, background(np.random.RandomState(len(name)), w, h), g['true_vps'], horizon


def flatten(c, guard=0, fill=0):
    """A case as the entry points take it: (dims int64 batch x 2 as (W, H), pix_offsets, rgb bytes, prim_offsets, geom, rgba,
    width), with ``guard`` bytes of ``fill`` behind every image."""
    dims = np.array([[im.shape[1], im.shape[0]] for im in c['images']], dtype=np.int64)
    chunks, pix = [], [0]
    for im in c['images']:
        chunks += [im.reshape(-1), np.full(guard, fill, np.uint8)]
        pix.append(pix[-1] + im.size + guard)
    cols = 2 if c['disc'] else 4
    off = np.concatenate(([0], np.cumsum([p[2].size for p in c['prims']]))).astype(np.int64)
    geom = np.ascontiguousarray(np.concatenate([p[0].reshape(-1, cols) for p in c['prims']]), dtype=np.float64)
    rgba = np.ascontiguousarray(np.concatenate([p[1].reshape(-1, 4) for p in c['prims']]), dtype=np.uint8)
    width = np.ascontiguousarray(np.concatenate([p[2] for p in c['prims']]), dtype=np.float64)
    return dims, np.array(pix, dtype=np.int64), np.ascontiguousarray(np.concatenate(chunks)), off, geom, rgba, width


def check_case(name, rgb, pix, guard=0, fill=0):
    """``rgb`` / ``pix``: the byte buffer after the blend and its offsets (flatten's layout).  Every image by ``check``, every
    guard byte untouched; the order pair differs, the outside case is unchanged."""
    c, refs = case(name), reference(name)
    for b, (im, ref) in enumerate(zip(c['images'], refs)):
        got = rgb[pix[b]:pix[b] + im.size].reshape(im.shape)
        check(got, ref, exact=c['exact'])
        assert (rgb[pix[b] + im.size:pix[b + 1]] == fill).all(), "guard bytes behind image %d were written" % b
        if name == "outside":
            assert np.array_equal(got, im)
    if name == "order_ab":
        assert not np.array_equal(reference("order_ab")[0]['rgb'], reference("order_ba")[0]['rgb'])
    drawn = refs[0]['drawn']
    if name == "bbox_only":
        assert drawn[:16, :16].any() and drawn[16:, 16:32].any() and not drawn[16:, :16].any()
    if name == "wide_four_tiles":
        assert drawn[:16, :16].any() and drawn[:16, 16:].any() and drawn[16:, :16].any() and drawn[16:, 16:].any()
    if name == "zero_length":
        assert drawn[16:, :16].any() and drawn[:16, :16].any()
