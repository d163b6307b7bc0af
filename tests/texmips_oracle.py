"""A numpy restatement of the mip chains of TextureCompressor::compress with generate_mipmaps (renderer/editor/render_plugins.cpp:165-215,
:324-401), independent of csrc/lmx_texmips.h: the coefficient builder, the three modes of computeMip, computeCoverage / scaleCoverage and the
loop that strings them together. DESIGN.md §4.24 is the contract.

  * stochastic (downsampleNormal) and coverage: the reference's arithmetic, bit for bit; the generator is stepped draw by draw here, where
    the library enters its stream by a closed form.
  * filtered: the resampler the library defines - stb_image_resize2's filter, sums in ascending source index, horizontal pass first - in
    float32 operation by operation (numpy never fuses a multiply with an add).

`mutant` names one rule to break (MUTANTS): the tests show that the fixture tells each of them.
"""
import math

import numpy as np

F = np.float32
LINEAR, SRGB, STOCHASTIC = 0, 1, 2
MAX_TAPS = 14
SMALL = F(2.0 ** -120)
MUTANTS = ("vertical_first", "no_edge_fold", "no_normalisation", "no_premultiplied", "draws_swapped", "coverage_per_image", "next_from_unscaled")


def levels(w, h):
    return max(w, h).bit_length()


def sizes(w, h):
    return [(max(w >> m, 1), max(h >> m, 1)) for m in range(levels(w, h))]


def _srgb_to_linear64(c):
    return c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4)


_tables = {}


def tables():
    """(decode[256], encode[256]): the linear value of an sRGB byte as stb tabulates it - the fp32 formula (its power, base and exponent
    fp32, taken in fp64 and rounded to fp32) rounded to six decimals; encode[k] = the fp64 linear value of (k - 0.5) / 255, rounded to fp32"""
    if not _tables:
        dec, enc = np.zeros(256, F), np.zeros(256, F)
        for i in range(256):
            c = F(i) / F(255.0)
            v = c / F(12.92) if c <= F(0.04045) else F(math.pow(float((c + F(0.055)) / F(1.055)), float(F(2.4))))
            dec[i] = F(math.floor(float(v) * 1e6 + 0.5) / 1e6)
        for k in range(1, 256):
            enc[k] = F(_srgb_to_linear64((k - 0.5) / 255.0))
        dec.setflags(write=False)
        enc.setflags(write=False)
        _tables["t"] = (dec, enc)
    return _tables["t"]


def mitchell(x):
    x = F(abs(x))
    if x < F(1.0):
        return (F(16.0) + x * x * (F(21.0) * x - F(36.0))) / F(18.0)
    if x < F(2.0):
        return (F(32.0) + x * (F(-60.0) + x * (F(36.0) - F(7.0) * x))) / F(18.0)
    return F(0.0)


_coeffs = {}


def coeffs(n_in, n_out, mutant=None):
    """-> (n0[n_out], n[n_out], c[n_out, MAX_TAPS] float32)"""
    key = (n_in, n_out, mutant if mutant in ("no_edge_fold", "no_normalisation") else None)
    if key in _coeffs:
        return _coeffs[key]
    n0, n, c = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros((n_out, MAX_TAPS), F)
    if n_in == n_out:
        n0[:], n[:], c[:, 0] = np.arange(n_out), 1, F(1.0)
    else:
        scale = F(n_out) / F(n_in)
        radius = F(2.0) / scale
        margin = int(np.ceil(F(4.0) / scale)) // 2
        for p in range(-margin, n_in + margin):
            pc = F(p) + F(0.5)
            first = max(int(np.floor((pc - radius) * scale + F(0.5))), 0)
            last = min(int(np.floor((pc + radius) * scale - F(0.5))), n_out - 1)
            if key[2] == "no_edge_fold" and not 0 <= p < n_in:
                continue
            texel = min(max(p, 0), n_in - 1)
            for o in range(first, last + 1):
                weight = mitchell((F(o) + F(0.5)) - pc * scale) * scale
                if n[o] == 0:
                    n0[o] = texel
                k = texel - n0[o]
                assert 0 <= k < MAX_TAPS, (n_in, n_out, o, k)
                c[o, k] = c[o, k] + weight
                n[o] = max(n[o], k + 1)
        assert (n > 0).all()
        if key[2] != "no_normalisation":
            for o in range(n_out):
                total = F(0.0)
                for k in range(n[o]):
                    total = total + c[o, k]
                inv = F(1.0) / total
                c[o, : n[o]] = c[o, : n[o]] * inv
    for v in (n0, n, c):
        v.setflags(write=False)
    _coeffs[key] = (n0, n, c)
    return _coeffs[key]


def _pass(chan, axis, table):
    """one pass along `axis` (0: rows, 1: columns) of chan (h, w, 7): sums in ascending source index from 0.0f"""
    n0, n, c = table
    size = chan.shape[axis]
    shape = (len(n0), chan.shape[1], 7) if axis == 0 else (chan.shape[0], len(n0), 7)
    acc = np.zeros(shape, F)
    for k in range(int(n.max())):
        idx = np.minimum(n0 + k, size - 1)
        coef = np.where(k < n, c[:, k], F(0.0)).astype(F)  # a tap past an output's last adds 0.0f * x: nothing
        acc = acc + (coef[:, None, None] * chan[idx] if axis == 0 else coef[None, :, None] * chan[:, idx])
    return acc


def _encode_linear(x):
    with np.errstate(invalid="ignore"):
        v = x * F(255.0) + F(0.5)
        return np.where(v > 0, np.where(v > 255, 255, np.where(np.isnan(v), 0, v)), 0).astype(np.uint8)  # truncation; a NaN gives 0


def _encode_srgb(x, enc):
    k = np.searchsorted(enc[1:], x, side="right")  # the k in 1 .. 255 with enc[k] <= x
    return np.where(np.isnan(x), 0, k).astype(np.uint8)


def filtered(src, dst_w, dst_h, srgb, mutant=None):
    """src uint8 (h, w, 4) -> uint8 (dst_h, dst_w, 4)"""
    h, w = src.shape[:2]
    dec, enc = tables()
    colour = dec[src[:, :, :3]] if srgb else src[:, :, :3].astype(F) * (F(1.0) / F(255.0))
    alpha = src[:, :, 3:].astype(F) * (F(1.0) / F(255.0))
    chan = np.concatenate([colour, alpha, colour * alpha], 2).astype(F)
    tx, ty = coeffs(w, dst_w, mutant), coeffs(h, dst_h, mutant)
    out = _pass(_pass(chan, 0, ty), 1, tx) if mutant == "vertical_first" else _pass(_pass(chan, 1, tx), 0, ty)
    a = out[:, :, 3:4]
    with np.errstate(all="ignore"):
        weighted = out[:, :, 4:] * (F(1.0) / a)
    rgb = np.where(a < SMALL, out[:, :, :3], weighted) if mutant != "no_premultiplied" else out[:, :, :3]
    rgb8 = _encode_srgb(rgb, enc) if srgb else _encode_linear(rgb)
    return np.concatenate([rgb8, _encode_linear(a)], 2)


def _rand(state):
    u, v = state
    u = (36969 * (u & 65535) + (u >> 16)) & 0xFFFFFFFF
    v = (18000 * (v & 65535) + (v >> 16)) & 0xFFFFFFFF
    state[0], state[1] = u, v
    return ((u << 16) + v) & 0xFFFFFFFF


def stochastic_indices(w, h, dst_w, dst_h, mutant=None):
    """downsampleNormal's (isrc, jsrc), int64 (dst_h, dst_w) each; every row steps its own generator, two draws per pixel"""
    rw, rh = F(w) / F(dst_w), F(h) / F(dst_h)
    j = np.arange(dst_h, dtype=np.int64)
    state = [np.full(dst_h, 521288629, np.uint64), ((362436069 + 1337 * j) & 0xFFFFFFFF).astype(np.uint64)]
    isrc, jsrc = np.zeros((dst_h, dst_w), np.int64), np.zeros((dst_h, dst_w), np.int64)

    def draw(to):
        return (np.float64(to) * (_rand(state).astype(np.float64) * 2.328306435996595e-10)).astype(F)

    def pick(r, s):
        whole = np.floor(s).astype(F)  # f - u32(f), f >= 0
        r0 = F(1.0) - (s - whole)
        return whole.astype(np.int64) + (r > r0).astype(np.int64) + (r > (r0 + F(1.0))).astype(np.int64)

    sj = j.astype(F) * rh
    for i in range(dst_w):
        if mutant == "draws_swapped":
            rc, rr = draw(rw), draw(rh)
        else:
            rr, rc = draw(rh), draw(rw)
        jsrc[:, i] = pick(rr, sj)
        isrc[:, i] = pick(rc, np.full(dst_h, F(i) * rw, F))
    return isrc, jsrc


def stochastic(src, dst_w, dst_h, mutant=None):
    h, w = src.shape[:2]
    isrc, jsrc = stochastic_indices(w, h, dst_w, dst_h, mutant)
    assert isrc.max() < w and jsrc.max() < h
    return src[jsrc, isrc]


def compute_mip(src, dst_w, dst_h, mode, mutant=None):
    if mode == STOCHASTIC:
        return stochastic(src, dst_w, dst_h, mutant)
    return filtered(src, dst_w, dst_h, mode == SRGB, mutant)


def _u8_clamped(v):
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.where(v > 255, 255, np.where(np.isnan(v), 0, v)), 0).astype(np.uint8)


def coverage_ref(ref_norm):
    return int(_u8_clamped(np.asarray(F(255) * F(ref_norm))))


def compute_coverage(img, ref_norm):
    count = int((img[:, :, 3] > coverage_ref(ref_norm)).sum())
    return F(np.float64(count) / np.float64(img.shape[0] * img.shape[1]))


def coverage_scale(img, ref_norm, wanted):
    """scaleCoverage's factor (:337-352); may be inf or NaN"""
    hist = np.bincount(img[:, :, 3].reshape(-1), minlength=256)
    count = int(F(img.shape[0] * img.shape[1]) * (F(1) - F(wanted)))
    new_ref = F(0)
    while new_ref < 255:
        b = int(hist[int(new_ref)])
        if count < b:
            new_ref = new_ref + F(count) / F(b)
            break
        count -= b
        new_ref = new_ref + F(1)
    with np.errstate(all="ignore"):
        return F(ref_norm) / (new_ref / F(255.0))


def scale_coverage(img, ref_norm, wanted):
    out = img.copy()
    with np.errstate(all="ignore"):
        out[:, :, 3] = _u8_clamped(img[:, :, 3].astype(F) * coverage_scale(img, ref_norm, wanted))  # 0 * inf, 0 / 0: the library writes 0
    return out


def chains(images, mode, scale_coverage_ref=-1.0, mutant=None):
    """images uint8 (n, h, w, 4) -> per image the list of its levels, level 0 included"""
    images = np.asarray(images, np.uint8)
    n, h, w = images.shape[:3]
    on = scale_coverage_ref >= 0
    wanted = compute_coverage(images[0], scale_coverage_ref) if on else None
    out = []
    for img in images:
        if on and mutant == "coverage_per_image":
            wanted = compute_coverage(img, scale_coverage_ref)
        chain, prev = [img], img
        for dw, dh in sizes(w, h)[1:]:
            mip = compute_mip(prev, dw, dh, mode, mutant)
            scaled = scale_coverage(mip, scale_coverage_ref, wanted) if on else mip
            chain.append(scaled)
            prev = mip if mutant == "next_from_unscaled" else scaled
        out.append(chain)
    return out


def flatten(chain_list):
    """chains() -> uint8 (n, chain bytes), as lmx_texcomp_read_pixels lays them out"""
    return np.stack([np.concatenate([lv.reshape(-1) for lv in chain]) for chain in chain_list])
