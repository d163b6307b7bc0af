"""A numpy restatement of the texture compressor's contract (csrc/lmx_texcomp.h), vectorised over blocks.

BC1 is rgbcx's encode_bc1 (external/rgbcx/rgbcx.h:3501-3842) with two least-squares passes, check-2 selectors and a search over selector
histograms: by default all 969 (3 colours: 153) in lexicographic order, each trial replacing the state only if strictly better, so the
lowest index among the trials of least error wins. `order4` / `order3` replace that list for tests/test_texcomp_oracle_vs_ref.py alone:
a function from the blocks' histogram before the search, (N, 4) or (N, 3), to the histograms to try, (N, K, 4) or (N, K, 3), in order.
`mutant` changes one rule (tests/test_texcomp_cpu.py). fp32 throughout where the reference computes in fp32, no fused multiply-add.
"""
import numpy as np

F = np.float32
I = np.int32  # (every value fits: errors < 2^22, sort keys < 2^29; the packing of blocks widens to int64 itself)
L = np.int64

STATS = {"clamped": 0, "det0": 0}  # routes taken since import: roundings that left [0, 31] / [0, 63], least-squares systems of determinant 0

MUTANTS = ("nonstrict", "tie_high", "one_ls_pass", "mid_ge", "axis_initial", "no_solid", "three_on_equal")


def expand5(v):
    return (v << 3) | (v >> 2)


def expand6(v):
    return (v << 2) | (v >> 4)


def to5(v):
    v = v * 31 + 128
    return (v + (v >> 8)) >> 8


def to6(v):
    v = v * 63 + 128
    return (v + (v >> 8)) >> 8


# ---- tables, generated ---------------------------------------------------------------------------------------------------------------------
def hist4_list():
    return np.array([(a, b, c, 16 - a - b - c) for a in range(17) for b in range(17 - a) for c in range(17 - a - b)], I)


def hist3_list():
    return np.array([(a, b, 16 - a - b) for a in range(17) for b in range(17 - a)], I)


def hist_index(h):
    h = [int(x) for x in h]
    if len(h) == 4:
        return sum((16 - a + 1) * (16 - a + 2) // 2 for a in range(h[0])) + sum(16 - h[0] - b + 1 for b in range(h[1])) + h[2]
    return sum(16 - a + 1 for a in range(h[0])) + h[1]


W4 = np.array([(0, 0, 9), (1, 2, 4), (4, 2, 1), (9, 0, 0)], I)  # z00, z10, z11 of g_weight_vals4
W3 = np.array([(0, 0, 4), (4, 0, 0), (1, 1, 1)], I)


def selector_factors(h):
    """compute_selector_factors4/3 for histograms (..., 4) or (..., 3) -> iz00, iz10, iz11 (float32)"""
    w = W4 if h.shape[-1] == 4 else W3
    z = (h[..., :, None] * w).sum(-2)
    z00, z10, z11 = F(z[..., 0]), F(z[..., 1]), F(z[..., 2])
    det = z00 * z11 - z10 * z10
    scale = F(3.0) / F(255.0) if h.shape[-1] == 4 else F(2.0) / F(255.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        det = np.where(np.abs(det) < F(1e-8), F(0), scale / det).astype(F)
    return z11 * det, -z10 * det, z00 * det


def _match_table(size, half):
    ex = expand5 if size == 32 else expand6
    i = np.arange(256)
    lowest = np.full(256, 256)
    hi_t, lo_t, e_t = np.zeros(256, I), np.zeros(256, I), np.zeros(256, I)
    for lo in range(size):
        for hi in range(size):
            lo_e, hi_e = ex(lo), ex(hi)
            v = (hi_e + lo_e) // 2 if half else (hi_e * 2 + lo_e) // 3
            e = np.abs(v - i) + (abs(hi_e - lo_e) * 3) // 100
            take = (e < lowest) | ((e == lowest) & (lo == hi))
            hi_t[take], lo_t[take], e_t[take] = hi, lo, e[take]
            lowest = np.where(take, e, lowest)
    return np.stack([hi_t, lo_t, e_t], 1)


_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        mid5 = np.array([round((expand5(i) + expand5(i + 1)) / 2 / 255, 6) for i in range(31)] + [1e37]).astype(F)
        mid6 = np.array([round((expand6(i) + expand6(i + 1)) / 2 / 255, 6) for i in range(63)] + [1e37]).astype(F)
        _TABLES = dict(mid5=mid5, mid6=mid6, m5=_match_table(32, False), m6=_match_table(64, False), m5h=_match_table(32, True), m6h=_match_table(64, True))
    return _TABLES


# ---- pieces ----------------------------------------------------------------------------------------------------------------------------------
def pal4(e):
    p = np.zeros((len(e), 4, 3), I)
    p[:, 0] = np.stack([expand5(e[:, 0]), expand6(e[:, 1]), expand5(e[:, 2])], 1)
    p[:, 3] = np.stack([expand5(e[:, 3]), expand6(e[:, 4]), expand5(e[:, 5])], 1)
    p[:, 1] = (p[:, 0] * 2 + p[:, 3]) // 3
    p[:, 2] = (p[:, 3] * 2 + p[:, 0]) // 3
    return p


def pal3(e):
    p = np.zeros((len(e), 3, 3), I)
    p[:, 0] = np.stack([expand5(e[:, 0]), expand6(e[:, 1]), expand5(e[:, 2])], 1)
    p[:, 1] = np.stack([expand5(e[:, 3]), expand6(e[:, 4]), expand5(e[:, 5])], 1)
    p[:, 2] = (p[:, 0] + p[:, 1]) // 2
    return p


def _sq3(p, k, px):
    """the squared distance of every pixel to palette entry k (an index per pixel, or one for all): channel by channel, no small reductions"""
    out = 0
    for c in range(3):
        pc = p[:, :, c]
        d = (np.take_along_axis(pc, k, 1) if isinstance(k, np.ndarray) else pc[:, k: k + 1]) - px[:, :, c]
        out = out + d * d
    return out


def find_sels4(px, e):
    """bc1_find_sels4_check2_err without the early-out -> sels (N, 16), err (N,)"""
    p = pal4(e)
    d = p[:, 3] - p[:, 0]
    f = F(4.0) / (F(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) + F(.00000125))
    t = F(sum((px[:, :, c] - p[:, 0, c, None]) * d[:, c, None] for c in range(3)))
    sel = np.clip((t * f[:, None] + F(.5)).astype(I), 1, 3)
    err0, err1 = _sq3(p, sel - 1, px), _sq3(p, sel, px)
    best_sel = np.where(err0 == err1, np.where(sel == 1, 0, sel), np.where(err0 < err1, sel - 1, sel))
    return best_sel, np.minimum(err0, err1).sum(1)


def find_sels3(px, e):
    p = pal3(e)
    err0, err1, err2 = _sq3(p, 0, px), _sq3(p, 1, px), _sq3(p, 2, px)
    best, sel = err0, np.zeros(err0.shape, I)
    sel = np.where(err1 < best, 1, sel)
    best = np.minimum(best, err1)
    sel = np.where(err2 < best, 2, sel)
    return sel, np.minimum(best, err2).sum(1)


def _solve(iz00, iz01, iz10, iz11, uq, q10):
    """(N,) factors, (N, 3) right-hand sides -> xl, xh"""
    xl = iz00[:, None] * uq + iz01[:, None] * q10
    xh = iz10[:, None] * uq + iz11[:, None] * q10
    return xl.astype(F), xh.astype(F)


def ls_from_sels(px, sels, total, four):
    w = (W4 if four else W3)[sels].sum(1)
    tsel = sels if four else np.array([0, 2, 1])[sels]
    uq = (tsel[:, :, None] * px).sum(1)
    q10 = total * (3 if four else 2) - uq
    z00, z10, z11 = F(w[:, 0]), F(w[:, 1]), F(w[:, 2])
    det = z00 * z11 - z10 * z10
    ok = ~(np.abs(det) < F(1e-8))
    STATS["det0"] += int((~ok).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        det = ((F(3.0) / F(255.0) if four else F(2.0) / F(255.0)) / det).astype(F)
        xl, xh = _solve(z11 * det, -z10 * det, -z10 * det, z00 * det, F(uq), F(q10))
    return ok, xl, xh


def ls_from_sums(sums, total, h):
    """sums (N, 17, 3), h (N, 4) or (N, 3) -> xl, xh"""
    n = np.arange(len(h))
    if h.shape[1] == 4:
        f1, f2, f3 = h[:, 0], h[:, 0] + h[:, 1], h[:, 0] + h[:, 1] + h[:, 2]
        uq = (sums[n, f2] - sums[n, f1]) + (sums[n, f3] - sums[n, f2]) * 2 + (total - sums[n, f3]) * 3
        q10 = total * 3 - uq
    else:
        f1, f2 = h[:, 0], h[:, 0] + h[:, 2]
        uq = (total - sums[n, f2]) * 2 + (sums[n, f2] - sums[n, f1])
        q10 = total * 2 - uq
    iz00, iz10, iz11 = selector_factors(h)
    return _solve(iz00, iz10, iz10, iz11, F(uq), F(q10))


def round565(xl, xh, mid_ge=False):
    """precise_round_565: the HIGH endpoint from xl, the LOW one from xh -> (N, 6) lr lg lb hr hg hb"""
    t = tables()

    def one(x, top, mid):
        with np.errstate(invalid="ignore", over="ignore"):  # (not finite where the determinant was 0: the caller takes the single-colour match there)
            v = (x * F(top)).astype(I)
        STATS["clamped"] += int((((v < 0) | (v > top)) & np.isfinite(x)).sum())
        v = np.where(v < 0, 0, np.where(v > top, top, v))
        up = (x >= mid[v]) if mid_ge else (x > mid[v])
        return (v + up) & top

    def three(x):
        return [one(x[:, 0], 31, t["mid5"]), one(x[:, 1], 63, t["mid6"]), one(x[:, 2], 31, t["mid5"])]

    return np.stack(three(xh) + three(xl), 1)


def match_endpoints(avg, four):
    t = tables()
    m5, m6 = (t["m5"], t["m6"]) if four else (t["m5h"], t["m6h"])
    r, g, b = m5[avg[:, 0]], m6[avg[:, 1]], m5[avg[:, 2]]
    return np.stack([r[:, 0], g[:, 0], b[:, 0], r[:, 1], g[:, 1], b[:, 1]], 1)


def pick_initial(px, avg):
    n = len(px)
    r, g, b = px[:, :, 0], px[:, :, 1], px[:, :, 2]
    grey = ((r == g) & (r == b)).all(1)
    mn, mx = px.min(1), px.max(1)
    e = np.zeros((n, 6), I)
    # greyscale
    narrow = (mx[:, 0] - mn[:, 0]) < 2
    lo = np.where(narrow, px[:, 0, 0], mn[:, 0])
    hi = np.where(narrow, px[:, 0, 0], mx[:, 0])
    eg = np.stack([to5(lo), to6(lo), to5(lo), to5(hi), to6(hi), to5(hi)], 1)
    # covariance and four power iterations
    c = px - avg[:, None]
    icov = [(c[:, :, i] * c[:, :, j]).sum(1) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    x = [F(mx[:, k] - mn[:, k]) for k in range(3)]
    x[0] = np.where(icov[2] < 0, -x[0], x[0])
    x[1] = np.where(icov[4] < 0, -x[1], x[1])
    cov = [F(v) * (F(1.0) / F(255.0)) for v in icov]
    for _ in range(4):
        nr = x[0] * cov[0] + x[1] * cov[1] + x[2] * cov[2]
        ng = x[0] * cov[1] + x[1] * cov[3] + x[2] * cov[4]
        nb = x[0] * cov[2] + x[1] * cov[4] + x[2] * cov[5]
        x = [nr, ng, nb]
    k = np.maximum(np.maximum(np.abs(x[0]), np.abs(x[1])), np.abs(x[2]))
    big = k >= 2
    with np.errstate(divide="ignore", invalid="ignore"):
        m = F(2048.0) / np.where(big, k, F(1))
    sax = [np.where(big, (x[i] * m).astype(I), d) << 4 for i, d in enumerate((306, 601, 117))]
    dot = ((r * sax[0][:, None] + g * sax[1][:, None] + b * sax[2][:, None]) & ~0xF) + np.arange(16)
    lo_c, hi_c = dot.min(1) & 15, dot.max(1) & 15
    idx = np.arange(n)
    pl, ph = px[idx, lo_c], px[idx, hi_c]
    ec = np.stack([to5(pl[:, 0]), to6(pl[:, 1]), to5(pl[:, 2]), to5(ph[:, 0]), to6(ph[:, 1]), to5(ph[:, 2])], 1)
    return np.where(grey[:, None], eg, ec)


def sorted_sums(px, e):
    """the prefix sums of the block sorted along the endpoints' axis -> (N, 17, 3)"""
    ax = np.stack([expand5(e[:, 3]) - expand5(e[:, 0]), expand6(e[:, 4]) - expand6(e[:, 1]), expand5(e[:, 5]) - expand5(e[:, 2])], 1)
    key = ((0x1000000 + (px * ax[:, None]).sum(2)) << 4) + np.arange(16)
    order = np.argsort(key, 1)
    srt = np.take_along_axis(px, order[:, :, None], 1)
    return np.concatenate([np.zeros((len(px), 1, 3), I), np.cumsum(srt, 1)], 1)


def refine(px, total, avg, first, four, mutant=None):
    """up to two least-squares passes from `first` -> e, sels, err"""
    find = find_sels4 if four else find_sels3
    e = first.copy()
    sels, err = find(px, e)
    alive = np.ones(len(px), bool) if four else err != 0
    for _ in range(1 if mutant == "one_ls_pass" else 2):
        ok, xl, xh = ls_from_sels(px, sels, total, four)
        trial = np.where(ok[:, None], round565(xl, xh, mutant == "mid_ge"), match_endpoints(avg, four))
        alive = alive & ~(trial == e).all(1)
        tsels, terr = find(px, trial)
        better = alive & (terr < err)
        e = np.where(better[:, None], trial, e)
        sels = np.where(better[:, None], tsels, sels)
        err = np.where(better, terr, err)
        alive = better
    return e, sels, err


def search(px, total, avg, e, sels, err, axis_e, hists, four, mutant=None):
    """hists (N, K, 4 | 3): the trials in order; a trial replaces the state if strictly better"""
    find = find_sels4 if four else find_sels3
    sums = sorted_sums(px, axis_e)
    active = err != 0
    replaced = np.zeros(len(px), bool)
    single = match_endpoints(avg, four)
    for q in range(hists.shape[1]):
        h = hists[:, q]
        xl, xh = ls_from_sums(sums, total, h)
        trial = np.where((h == 16).any(1)[:, None], single, round565(xl, xh, mutant == "mid_ge"))
        tsels, terr = find(px, trial)
        better = terr < err
        if mutant == "nonstrict":
            better = terr <= err
        elif mutant == "tie_high":
            better = better | (replaced & (terr == err))
        better &= active
        replaced |= better
        e = np.where(better[:, None], trial, e)
        sels = np.where(better[:, None], tsels, sels)
        err = np.where(better, terr, err)
    return e, sels, err


def _pack(e):
    e = e.astype(L)
    return e[:, 2] | (e[:, 1] << 5) | (e[:, 0] << 11), e[:, 5] | (e[:, 4] << 5) | (e[:, 3] << 11)


def _bytes(w0, w1):
    return np.stack([w0.astype(np.uint32), w1.astype(np.uint32)], 1).astype("<u4").view(np.uint8).reshape(-1, 8)


def _sel_bits(s):
    return (s.astype(L) << (2 * np.arange(16))).sum(1)


def encode4(e, sels):
    lc, hc = _pack(e)
    same = lc == hc
    swap = lc < hc
    packed = _sel_bits(np.array([0, 2, 3, 1])[sels]) ^ np.where(swap, 0x55555555, 0)
    lo, hi = np.where(swap, hc, lc), np.where(swap, lc, hc)
    # equal endpoints: never a 3-colour block
    lo = np.where(same, np.where(hc > 0, lc, 1), lo)
    hi = np.where(same, np.where(hc > 0, hc - 1, 0), hi)
    packed = np.where(same, np.where(hc > 0, 0, 0x55555555), packed)
    return _bytes(lo | (hi << 16), packed)


def encode3(e, sels):
    lc, hc = _pack(e)
    swap = lc > hc
    s = np.where(swap[:, None], np.array([1, 0, 2, 3])[sels], sels)
    return _bytes(np.where(swap, hc, lc) | (np.where(swap, lc, hc) << 16), _sel_bits(s))


def solid_block(c, allow3):
    t = {k: v.astype(L) for k, v in tables().items() if k[0] == "m" and k[1] != "i"}
    r4, g4, b4 = t["m5"][c[:, 0]], t["m6"][c[:, 1]], t["m5"][c[:, 2]]
    r3, g3, b3 = t["m5h"][c[:, 0]], t["m6h"][c[:, 1]], t["m5h"][c[:, 2]]
    mx4, mn4 = (r4[:, 0] << 11) | (g4[:, 0] << 5) | b4[:, 0], (r4[:, 1] << 11) | (g4[:, 1] << 5) | b4[:, 1]
    mask = np.full(len(c), 0xAA)
    eq = mn4 == mx4
    mask = np.where(eq, np.where(mn4 > 0, 0, 0x55), mask)
    mx = np.where(eq & (mn4 == 0), 1, mx4)
    mn = np.where(eq & (mn4 > 0), mn4 - 1, np.where(eq, 0, mn4))
    sw = mx < mn
    mask = np.where(sw, mask ^ 0x55, mask)
    mx, mn = np.where(sw, mn, mx), np.where(sw, mx, mn)
    if allow3:
        use3 = (r3[:, 2] + g3[:, 2] + b3[:, 2]) < (r4[:, 2] + g4[:, 2] + b4[:, 2])
        mx3, mn3 = (r3[:, 0] << 11) | (g3[:, 0] << 5) | b3[:, 0], (r3[:, 1] << 11) | (g3[:, 1] << 5) | b3[:, 1]
        lo3, hi3 = np.minimum(mx3, mn3), np.maximum(mx3, mn3)  # color0 <= color1: a 3-colour block, every selector 2
        mx, mn, mask = np.where(use3, lo3, mx), np.where(use3, hi3, mn), np.where(use3, 0xAA, mask)
    return _bytes(mx | (mn << 16), mask * 0x01010101)


def encode_bc1_pair(rgba, order4=None, order3=None, mutant=None):
    """rgba: uint8 (N, 16, 4) -> (bytes, err) without 3-colour blocks and (bytes, err) with them allowed; bytes uint8 (N, 8), err (N,): the
    encoder's own squared error (0 where the solid shortcut was taken). The 4-colour search is shared."""
    assert mutant is None or mutant in MUTANTS
    px = np.asarray(rgba)[:, :, :3].astype(I)
    n = len(px)
    solid = (px == px[:, :1]).all((1, 2))
    if mutant == "no_solid":
        solid = np.zeros(n, bool)
    total = px.sum(1, dtype=I)
    avg = (total + 8) >> 4
    first = pick_initial(px, avg)
    e4, s4, err4 = refine(px, total, avg, first, True, mutant)
    hist = np.stack([(s4 == k).sum(1) for k in range(4)], 1)
    trials = np.broadcast_to(hist4_list(), (n, 969, 4)) if order4 is None else order4(hist)
    e4, s4, err4 = search(px, total, avg, e4, s4, err4, first if mutant == "axis_initial" else e4, trials, True, mutant)
    out4 = encode4(e4, s4)
    e3, s3, err3 = refine(px, total, avg, first, False, mutant)
    hist = np.stack([(s3 == k).sum(1) for k in range(3)], 1)
    trials = np.broadcast_to(hist3_list(), (n, 153, 3)) if order3 is None else order3(hist)
    e3, s3, err3 = search(px, total, avg, e3, s3, err3, first if mutant == "axis_initial" else e3, trials, False, mutant)
    three = (err4 != 0) & ((err3 <= err4) if mutant == "three_on_equal" else (err3 < err4))
    out3 = np.where(three[:, None], encode3(e3, s3), out4)
    err3 = np.where(three, err3, err4)
    res = []
    for out, err, allow3 in ((out4, err4, False), (out3, err3, True)):
        out = np.where(solid[:, None], solid_block(px[:, 0], allow3), out)
        res.append((out.astype(np.uint8), np.where(solid, 0, err).astype(np.uint32)))
    return res


def encode_bc1(rgba, allow3, order4=None, order3=None, mutant=None):
    return encode_bc1_pair(rgba, order4, order3, mutant)[1 if allow3 else 0]


def encode_bc4(v):
    """encode_bc4 of values uint8 (N, 16) -> uint8 (N, 8)"""
    v = np.asarray(v).astype(L)
    mn, mx = v.min(1), v.max(1)
    delta = (mx - mn)[:, None]
    x = v * 14 + (4 - mn * 14)[:, None]
    cnt = sum((x >= delta * k).astype(I) for k in (13, 11, 9, 7, 5, 3, 1))
    sel = np.array([1, 7, 6, 5, 4, 3, 2, 0])[cnt]
    bits = np.where((mx == mn)[:, None], 0, sel << (3 * np.arange(16))).sum(1)
    return np.concatenate([np.stack([mx, mn], 1).astype(np.uint8), bits.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :6]], 1)


BC1, BC3, BC4, BC5 = 0, 1, 2, 3


def encode(rgba, fmt):
    """blocks uint8 (N, 16, 4) -> (bytes (N, 8 | 16), the BC1 half's error (N,) or None)"""
    rgba = np.asarray(rgba, np.uint8).reshape(-1, 16, 4)
    if fmt == BC1:
        return encode_bc1(rgba, True)
    if fmt == BC3:
        c, err = encode_bc1(rgba, False)
        return np.concatenate([encode_bc4(rgba[:, :, 3]), c], 1), err
    if fmt == BC4:
        return encode_bc4(rgba[:, :, 0]), None
    return np.concatenate([encode_bc4(rgba[:, :, 0]), encode_bc4(rgba[:, :, 1])], 1), None


# ---- what the tests measure with -------------------------------------------------------------------------------------------------------------
def decode_bc1(blocks):
    """the ideal decode of BC1 blocks uint8 (N, 8) -> rgb (N, 16, 3), and which blocks are 3-colour"""
    w = np.ascontiguousarray(blocks, np.uint8).view("<u2").reshape(-1, 4).astype(L)
    c0, c1 = w[:, 0], w[:, 1]

    def rgb(c):
        return np.stack([expand5(c >> 11), expand6((c >> 5) & 63), expand5(c & 31)], 1)

    p0, p1 = rgb(c0), rgb(c1)
    four = c0 > c1
    p2 = np.where(four[:, None], (p0 * 2 + p1) // 3, (p0 + p1) // 2)
    p3 = np.where(four[:, None], (p1 * 2 + p0) // 3, 0)
    pal = np.stack([p0, p1, p2, p3], 1)
    bits = (w[:, 2] | (w[:, 3] << 16))[:, None] >> (2 * np.arange(16)) & 3
    return pal[np.arange(len(w))[:, None], bits], ~four


def block_error(rgba, blocks):
    """the squared RGB difference of BC1 blocks to their pixels under the ideal decode"""
    dec, _ = decode_bc1(blocks)
    return ((dec - np.asarray(rgba)[:, :, :3].astype(L)) ** 2).sum((1, 2))


def image_blocks(img):
    """uint8 (h, w, 4) -> its 4 x 4 blocks in row-major block order, (n, 16, 4); texels outside the image are 0, 0, 0, 0"""
    h, w = img.shape[:2]
    bh, bw = (h + 3) >> 2, (w + 3) >> 2
    pad = np.zeros((bh * 4, bw * 4, 4), np.uint8)
    pad[:h, :w] = img
    return pad.reshape(bh, 4, bw, 4, 4).transpose(0, 2, 1, 3, 4).reshape(bh * bw, 16, 4)


def fixture_blocks():
    """The blocks of tests/golden/texcomp_small.npz (at most 2048): five seeded kinds and the edge cases of the issue; uint8 (N, 16, 4)."""
    rng = np.random.default_rng(20261021)
    out = []
    k = 300
    out.append(rng.integers(0, 256, (k, 16, 4)))  # noise
    a, b = rng.integers(0, 256, (k, 1, 4)), rng.integers(0, 256, (k, 1, 4))
    t = rng.random((k, 16, 1))
    out.append(np.clip(a + (b - a) * t + rng.normal(0, 6, (k, 16, 4)), 0, 255))  # noisy gradients
    out.append(np.clip(rng.integers(0, 256, (k, 1, 4)) + rng.integers(-2, 3, (k, 16, 4)), 0, 255))  # near-flat
    g0, g1 = rng.integers(0, 256, (k, 1, 1)), rng.integers(0, 256, (k, 1, 1))
    out.append(np.broadcast_to(np.where(np.arange(16)[None, :, None] < 8, g0, g1), (k, 16, 4)))  # two grey halves
    pick = rng.integers(0, 2, (k, 16, 1))
    out.append(np.where(pick == 1, a, b))  # two colours
    # solid blocks: black, white, every grey level, colours whose matched endpoints coincide
    solid = [(0, 0, 0), (255, 255, 255), (8, 4, 8), (1, 1, 1), (255, 0, 0), (0, 255, 0), (0, 0, 255), (33, 65, 33), (123, 125, 123)] + [(v, v, v) for v in range(0, 256, 5)]
    solid += [tuple(int(x) for x in rng.integers(0, 256, 3)) for _ in range(60)]
    out.append(np.array([[list(c) + [255]] * 16 for c in solid]))
    # greyscale with a range below 2, and of 2 and more
    base = rng.integers(0, 255, (40, 1, 1))
    out.append(np.broadcast_to(base + rng.integers(0, 2, (40, 16, 1)), (40, 16, 4)))
    out.append(np.broadcast_to(np.clip(base + rng.integers(0, 40, (40, 16, 1)), 0, 255), (40, 16, 4)))
    # one pixel off a solid block: a determinant of 0 after the first selectors, all but one selector equal
    one_off = np.broadcast_to(rng.integers(0, 256, (40, 1, 4)), (40, 16, 4)).copy()
    one_off[np.arange(40), rng.integers(0, 16, 40), rng.integers(0, 3, 40)] ^= 1
    out.append(one_off)
    # dark pixels among bright ones
    dark = rng.integers(100, 256, (60, 16, 4))
    low = rng.random((60, 16)) < 0.3
    dark[low] = rng.integers(0, 4, (int(low.sum()), 4))
    out.append(dark)
    # extremes: least squares overshoots [0, 1] where most pixels sit at 0 / 255 and a few in between
    ext = np.where(rng.random((120, 16, 4)) < 0.5, 0, 255)
    mid = rng.random((120, 16)) < 0.25
    ext[mid] = rng.integers(0, 256, (int(mid.sum()), 4))
    out.append(ext)
    # BC4 (channels 0, 1 and 3 alike): flat, delta 1, 0 / 255, and values on every threshold (2 k + 1) delta / 14
    bc4 = [np.full(16, 77), np.array([7, 8] * 8), np.array([0, 255] * 8), np.array([0] * 15 + [255])]
    for lo, hi in ((0, 255), (10, 24), (3, 17), (100, 107), (0, 14), (50, 78), (200, 255)):
        d = hi - lo
        th = sorted({lo + ((2 * k + 1) * d + s) // 14 for k in range(7) for s in (0, 13)})
        vals = ([lo, hi] + th + [lo] * 16)[:16]
        bc4.append(np.array(vals))
    out.append(np.stack([np.stack([v, v[::-1], (v * 7) % 256, v], 1) for v in bc4]))
    blocks = np.concatenate([np.asarray(o).astype(np.uint8) for o in out])
    assert len(blocks) <= 2048
    return np.ascontiguousarray(blocks)
