"""The probe bake's contract in numpy: SphericalHarmonics::compute (renderer/editor/render_plugins.cpp:476-587) and the
reflection probe's three steps - the mip chain (the `downscale` program, :2850-2898), the radiance levels (data/shaders/ibl_filter.hlsl)
over the cube sampler that lmx_probes.h defines, and saveCubemap's RGBM bytes (:3555-3559) - in float32 and in the reference's operation order. Sequential sums are
np.add.accumulate in float32 (accumulate adds element after element; reduce would add pairwise). tests/test_probe_oracle_vs_ref.py holds
this file to the reference's own code; tests/test_probes_cpu.py shows that each rule written here is one the results depend on.

Every function takes `rules`, a set of names of rules to break (the mutants of tests/test_probes_cpu.py); the empty set is the contract."""
import numpy as np

F = np.float32
PI = F(3.14159265)  # core/math.h:404
CONTRACT = frozenset()
SH_MUTANTS = ("strided_sum", "pairwise_sum", "weight_from_2u_minus_1", "contracted_multiply_add", "true_division_in_normalize", "missing_v_flip", "filter_face_table",
              "mults_before_scale")
MIP_MUTANTS = ("mip_pairwise_sum", "mip_flush_subnormals")
SAMPLER_MUTANTS = ("clamped_seams", "ties_z_first", "no_half_texel", "mip_lerp_other_form")
FILTER_MUTANTS = ("dim_is_S", "roughness_off_by_one", "lod_without_clamp", "clamped_seams", "one_sample_dropped")
RGBM_MUTANTS = ("rgbm_without_half",)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _normalize(x, y, z, rules):
    s = np.sqrt((x * x + y * y) + z * z, dtype=F)
    if "true_division_in_normalize" in rules:
        return x / s, y / s, z / s
    inv = F(1) / s  # core/math.cpp:367-376: 1 / sqrtf, then three multiplies
    return x * inv, y * inv, z * inv


def sh_table(S, rules=CONTRACT):
    """-> (basis float32 (6 S^2, 9), weight float32 (6 S^2,)) in face, y, x order"""
    w = F(S)
    i = np.arange(S, dtype=np.uint32).astype(F)
    u01 = (i + F(0.5)) / w
    face, y, x = np.meshgrid(np.arange(6), np.arange(S), np.arange(S), indexing="ij")
    U, V = u01[x], u01[y]
    if "weight_from_2u_minus_1" in rules:
        U, V = U * F(2) - F(1), V * F(2) - F(1)
    temp = (F(1) + U * U) + V * V
    weight = F(4) / (np.sqrt(temp, dtype=F) * temp)
    u = u01[x] * F(2) - F(1)
    v = u01[y] * F(2) - F(1)
    if "missing_v_flip" not in rules:
        v = v * F(-1)
    one = np.ones_like(u)
    if "filter_face_table" in rules:  # ibl_filter.hlsl's `switch (u_face)` (:83-90) read with cube2dir's u and v as its uv
        table = [(one, -v, -u), (-one, -v, u), (u, one, v), (u, -one, -v), (u, -v, one), (-u, -v, -one)]
    else:  # cube2dir, :531-538
        table = [(one, v, -u), (-one, v, u), (u, one, -v), (u, -one, v), (u, v, one), (-u, v, -one)]
    dx, dy, dz = (np.empty_like(u) for _ in range(3))
    for f, (a, b, c) in enumerate(table):
        dx[f], dy[f], dz[f] = a[f], b[f], c[f]
    dx, dy, dz = _normalize(f32(dx), f32(dy), f32(dz), rules)
    b = np.empty((6, S, S, 9), F)
    b[..., 0] = F(0.282095)
    b[..., 1] = F(0.488603) * dy
    b[..., 2] = F(0.488603) * dz
    b[..., 3] = F(0.488603) * dx
    b[..., 4] = F(1.092548) * dx * dy
    b[..., 5] = F(1.092548) * dy * dz
    b[..., 6] = F(0.315392) * (F(3) * dz * dz - F(1))
    b[..., 7] = F(1.092548) * dx * dz
    b[..., 8] = F(0.546274) * (dx * dx - dy * dy)
    assert b.dtype == F and weight.dtype == F
    return b.reshape(-1, 9), f32(weight).reshape(-1)


def sh_mults():
    return np.array([F(0.282095), F(0.488603) * F(2) / F(3), F(0.488603) * F(2) / F(3), F(0.488603) * F(2) / F(3), F(1.092548) / F(4), F(1.092548) / F(4), F(0.315392) / F(4),
                     F(1.092548) / F(4), F(0.546274) / F(4)], F)


def _sum(terms, rules):
    """the sum over axis 0 as the rules say: element after element in float32 unless a mutant reorders it"""
    if "strided_sum" in rules:  # 64 lanes take every 64th element, then the lanes are added in order
        lanes = [np.add.accumulate(terms[k::64], axis=0, dtype=F)[-1] for k in range(min(64, len(terms)))]
        return np.add.accumulate(np.stack(lanes), axis=0, dtype=F)[-1]
    if "pairwise_sum" in rules:
        a = terms
        while len(a) > 1:
            if len(a) % 2:
                a = np.concatenate([a, np.zeros_like(a[:1])])
            a = a[0::2] + a[1::2]
        return a[0]
    return np.add.accumulate(terms, axis=0, dtype=F)[-1]


def sh_compute(pixels, rules=CONTRACT):
    """pixels: float32 (6, S, S, 4) -> float32 (9, 3)"""
    pixels = f32(pixels)
    S = pixels.shape[1]
    assert pixels.shape == (6, S, S, 4)
    basis, weight = sh_table(S, rules)
    color = pixels.reshape(-1, 4)[:, :3]
    cw = color * weight[:, None]  # color * weight
    if "contracted_multiply_add" in rules:  # sum = fma(b, cw, sum): the product unrounded (exact in float64), one rounding per add
        acc = np.zeros((9, 3), np.float64)
        b64, cw64 = basis.astype(np.float64), cw.astype(np.float64)
        for p in range(len(cw)):
            acc = (acc + b64[p][:, None] * cw64[p][None, :]).astype(F).astype(np.float64)
        total = acc.astype(F)
    else:
        terms = basis[:, :, None] * cw[:, None, :]  # Vec3(b_i) * (color * weight)
        assert terms.dtype == F
        total = _sum(terms, rules)
    weight_sum = _sum(weight, rules)
    scale = (F(4) * PI) / weight_sum
    if "mults_before_scale" in rules:
        return f32((total * sh_mults()[:, None]) * scale)
    return f32((total * scale) * sh_mults()[:, None])


def mip_chain(pixels, rules=CONTRACT):
    """pixels: float32 (6, S, S, 4), S a power of two -> [mip 1, ..., mip log2 S], each (6, s, s, 4)"""
    a = f32(pixels)
    out = []
    while a.shape[1] > 1:
        v00, v10, v01, v11 = a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]  # (i inner = x, j outer = y)
        if "mip_pairwise_sum" in rules:
            a = ((v00 + v10) + (v01 + v11)) * F(0.25)
        elif "mip_flush_subnormals" in rules:  # what D3D may do and this does not
            z = lambda t: np.where(np.abs(t) < np.finfo(F).tiny, F(0), t)
            a = z(((((F(0) + z(v00)) + z(v10)) + z(v01)) + z(v11)) * F(0.25))
        else:
            a = ((((F(0) + v00) + v10) + v01) + v11) * F(0.25)
        a = f32(a)
        out.append(a)
    return out


# ---- the cube sampler (lmx_probes.h: ours to define) ----------------------------------------------------------------------------------------
def _where3(cx, cy, vx, vy, vz):
    return np.where(cx, vx, np.where(cy, vy, vz))


def face_dir(face, a, b):
    """ibl_filter.hlsl's `switch (u_face)` with uv = (a, b), not normalized -> (x, y, z)"""
    one = np.ones_like(a)
    table = [(one, -b, -a), (-one, -b, a), (a, one, b), (a, -one, -b), (a, -b, one), (-a, -b, -one)]
    return tuple(np.choose(face, [t[k] for t in table]) for k in range(3))


def texel_dir(x, y, face, s, T=F):
    """the shader's direction of texel (x, y): mainVS's flip, in_uv, `uv.y *= -1`, the table"""
    a = ((x.astype(T) + T(0.5)) / T(s)) * T(2) - T(1)
    b = (T(1) - (y.astype(T) + T(0.5)) / T(s)) * T(2) - T(1)
    b = b * T(-1)
    return face_dir(face, a, b)


def dir_coord(dx, dy, dz, rules=CONTRACT):
    """direction -> (face, a, b): the major axis picks the face, ties in x, y, z order"""
    ax, ay, az = np.abs(dx), np.abs(dy), np.abs(dz)
    if "ties_z_first" in rules:
        cz = (az >= ax) & (az >= ay)
        cy = ~cz & (ay >= ax)
        cx = ~cz & ~cy
    else:
        cx = (ax >= ay) & (ax >= az)
        cy = ~cx & (ay >= az)
    face = _where3(cx, cy, np.where(dx < 0, 1, 0), np.where(dy < 0, 3, 2), np.where(dz < 0, 5, 4))
    with np.errstate(all="ignore"):
        a = _where3(cx, cy, np.where(dx < 0, dz, -dz) / ax, dx / ay, np.where(dz < 0, -dx, dx) / az)
        b = _where3(cx, cy, -dy / ax, np.where(dy < 0, -dz, dz) / ay, -dy / az)
    return face, a, b


def _texel(mip, face, x, y, rules, T):
    """mip: (6, s, s, 4) -> rgb (k, 3) in T; x, y may lie one texel outside the face"""
    s = mip.shape[1]
    if "clamped_seams" in rules:
        return mip[face, np.clip(y, 0, s - 1), np.clip(x, 0, s - 1), :3].astype(T)
    inside = (x >= 0) & (x < s) & (y >= 0) & (y < s)
    a = ((x.astype(T) + T(0.5)) / T(s)) * T(2) - T(1)
    b = ((y.astype(T) + T(0.5)) / T(s)) * T(2) - T(1)
    f2, a2, b2 = dir_coord(*face_dir(face, a, b), rules)
    xi = np.clip(np.floor((a2 + T(1)) * T(0.5) * T(s)).astype(np.int64), 0, s - 1)
    yi = np.clip(np.floor((b2 + T(1)) * T(0.5) * T(s)).astype(np.int64), 0, s - 1)
    f, xx, yy = np.where(inside, face, f2), np.where(inside, x, xi), np.where(inside, y, yi)
    return mip[f, yy, xx, :3].astype(T)


def _lerp(p, q, t):
    return p + (q - p) * t


def _bilinear(mip, face, a, b, rules, T):
    s = mip.shape[1]
    half = T(0.0) if "no_half_texel" in rules else T(0.5)
    fx = (a + T(1)) * T(0.5) * T(s) - half
    fy = (b + T(1)) * T(0.5) * T(s) - half
    x0 = np.clip(np.floor(fx).astype(np.int64) + 1, 0, s) - 1
    y0 = np.clip(np.floor(fy).astype(np.int64) + 1, 0, s) - 1
    tx, ty = (fx - x0.astype(T))[:, None], (fy - y0.astype(T))[:, None]
    t00, t10 = _texel(mip, face, x0, y0, rules, T), _texel(mip, face, x0 + 1, y0, rules, T)
    t01, t11 = _texel(mip, face, x0, y0 + 1, rules, T), _texel(mip, face, x0 + 1, y0 + 1, rules, T)
    return _lerp(_lerp(t00, t10, tx), _lerp(t01, t11, tx), ty)


def sample(chain, dirs, lods, rules=CONTRACT, T=F):
    """chain: [mip 0, ..., mip log2 S] of (6, s, s, 4) float32; dirs (k, 3), lods (k,) in T -> rgb (k, 3) in T: trilinear, a lod past the
    last mip reads the last mip"""
    dirs, lods = np.asarray(dirs, T).reshape(-1, 3), np.asarray(lods, T).reshape(-1)
    last = len(chain) - 1
    face, a, b = dir_coord(dirs[:, 0], dirs[:, 1], dirs[:, 2], rules)
    top = T(last)
    l = np.where(lods > 0, np.where(lods < top, lods, top), T(0))
    m0 = np.floor(l).astype(np.int64)
    m1 = np.minimum(m0 + 1, last)
    t = (l - m0.astype(T))[:, None]
    c0, c1 = np.zeros((len(l), 3), T), np.zeros((len(l), 3), T)
    for m in range(last + 1):
        for which, out in ((m0, c0), (m1, c1)):
            k = np.nonzero(which == m)[0]
            if len(k):
                out[k] = _bilinear(chain[m], face[k], a[k], b[k], rules, T)
    if "mip_lerp_other_form" in rules:
        return c0 * (T(1) - t) + c1 * t
    return _lerp(c0, c1, t)


# ---- the radiance filter (data/shaders/ibl_filter.hlsl) -------------------------------------------------------------------------------------
M_PI = 3.14159265359  # common.hlsli:10


def radical_inverse(i):
    bits = np.asarray(i, np.uint32)
    bits = (bits << np.uint32(16)) | (bits >> np.uint32(16))
    for mask, sh in ((0x55555555, 1), (0x33333333, 2), (0x0F0F0F0F, 4), (0x00FF00FF, 8)):
        bits = ((bits & np.uint32(mask)) << np.uint32(sh)) | ((bits & np.uint32(~mask & 0xFFFFFFFF)) >> np.uint32(sh))
    return bits


def ggx_samples(level, T=F):
    """ImportanceSampleGGX's tangent-space H of the 128 Hammersley points at roughness level / 4 -> (128, 3) in T"""
    i = np.arange(128, dtype=np.uint32)
    xi_x = i.astype(T) / T(128)
    xi_y = radical_inverse(i).astype(T) * T(2.3283064365386963e-10)
    r = T(level) / T(4)
    a = r * r
    phi = T(2.0) * T(M_PI) * xi_x
    cos_t = np.sqrt((T(1) - xi_y) / (T(1) + (a * a - T(1)) * xi_y))
    sin_t = np.sqrt(T(1) - cos_t * cos_t)
    return np.stack([np.cos(phi) * sin_t, np.sin(phi) * sin_t, cos_t], axis=1).astype(T)


def _dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def _norm(v, T):
    inv = T(1) / np.sqrt(_dot(v, v))
    return (v[0] * inv, v[1] * inv, v[2] * inv)


def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def filter_samples(N, Ht, level, S, rules=CONTRACT, T=F):
    """mainPS's loop body for the normalized N (three arrays (k, 1)) and the table Ht (128, 3) -> (L: three (k, 128), NdotL, lod, gate)"""
    r_level = level + 1 if "roughness_off_by_one" in rules else level
    rough = T(r_level) / T(4)
    zero, one = np.zeros_like(N[0]), np.ones_like(N[0])
    flat = np.abs(N[2]) < T(0.999)
    up = (np.where(flat, zero, one), zero, np.where(flat, one, zero))
    tangent = _norm(_cross(up, N), T)
    bitangent = _cross(N, tangent)
    hx, hy, hz = Ht[None, :, 0], Ht[None, :, 1], Ht[None, :, 2]
    sv = tuple((tangent[k] * hx + bitangent[k] * hy) + N[k] * hz for k in range(3))
    H = _norm(sv, T)
    kk = T(2) * _dot(N, H)
    L = _norm(tuple(kk * H[k] - N[k] for k in range(3)), T)
    ndotl = _dot(N, L)
    ldoth, ndoth = _dot(L, H), _dot(N, H)
    a = rough * rough
    a2 = a * a
    f0 = (ndoth * ndoth) * (a2 - T(1)) + T(1)
    f = np.where(T(1e-5) > f0, T(1e-5), f0)
    with np.errstate(all="ignore"):
        D = a2 / (f * f * T(M_PI))
        ipdf = (T(4) * ldoth) / (D * ndoth)
        dim = T(S) if "dim_is_S" in rules else T(128)
        omega_p = (T(4) * T(M_PI)) / (T(6) * dim * dim)
        inv_omega_p = T(1) / omega_p
        omega_s = (T(1) / T(128)) * ipdf
        arg = T(4) * omega_s * inv_omega_p
        lod = np.log2(arg).astype(T) * T(0.5)
    if "lod_without_clamp" not in rules:
        lod = np.where(lod > 0, np.where(lod < T(4), lod, T(4)), T(0))
    return L, ndotl, lod.astype(T), ndotl > 0


def filter_level(chain, level, rules=CONTRACT, T=F, table=None):
    """level 1 .. 4 of the radiance filter -> (6, s, s, 4) in T"""
    S = chain[0].shape[1]
    s = S >> level
    face, y, x = (v.reshape(-1) for v in np.meshgrid(np.arange(6), np.arange(s), np.arange(s), indexing="ij"))
    N = _norm(texel_dir(x, y, face, s, T), T)
    N = tuple(v[:, None] for v in N)
    Ht = ggx_samples(level + 1 if "roughness_off_by_one" in rules else level, T) if table is None else np.asarray(table, T)
    L, ndotl, lod, gate = filter_samples(N, Ht, level, S, rules, T)
    if "one_sample_dropped" in rules:
        gate = gate.copy()
        gate[:, 77] = False
    dirs = np.stack([v.reshape(-1) for v in L], axis=1)
    col = np.zeros((dirs.shape[0], 3), T)
    k = np.nonzero(gate.reshape(-1))[0]
    col[k] = sample(chain, dirs[k], lod.reshape(-1)[k], rules, T)
    w = np.where(gate, ndotl, T(0))
    col = col.reshape(gate.shape + (3,)) * w[:, :, None]
    with np.errstate(all="ignore"):
        rgb = col.sum(axis=1, dtype=T) / w.sum(axis=1, dtype=T)[:, None]
    out = np.ones((6, s, s, 4), T)
    out[..., :3] = rgb.reshape(6, s, s, 3)
    return out


def level0(chain, rules=CONTRACT, T=F):
    """the shader's `u_mip == 0` branch: the cubemap sampled at each texel's own direction"""
    S = chain[0].shape[1]
    face, y, x = (v.reshape(-1) for v in np.meshgrid(np.arange(6), np.arange(S), np.arange(S), indexing="ij"))
    d = np.stack(texel_dir(x, y, face, S, T), axis=1)
    out = np.ones((6, S, S, 4), T)
    out[..., :3] = sample(chain, d, np.zeros(len(d), T), rules, T).reshape(6, S, S, 3)
    return out


def filter_levels(pixels, rules=CONTRACT, T=F):
    """pixels (6, S, S, 4) float32 -> levels 0 .. 4, each (6, s, s, 4) in T. The mip chain under the sampler is the float32 one."""
    chain = [f32(pixels)] + mip_chain(pixels, rules)
    return [level0(chain, rules, T)] + [filter_level(chain, k, rules, T) for k in range(1, 5)]


# ---- RGBM (saveCubemap's loop, :3555-3559) ---------------------------------------------------------------------------------------------------
def _max(a, b):
    return np.where(a > b, a, b)  # core/math.h: maximum(a, b) = a > b ? a : b


def _min(a, b):
    return np.where(a < b, a, b)


def _clamp(v, lo, hi):
    return _min(_max(v, lo), hi)


def rgbm_texels(rgb, rules=CONTRACT):
    """float32 (..., 3 or 4) -> uint8 (..., 4): r, g, b, m"""
    rgb = f32(rgb)
    x, y, z = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    half = F(0) if "rgbm_without_half" in rules else F(0.5)
    m = _clamp(_max(x, _max(y, z)), F(1) / F(64), F(4))
    with np.errstate(all="ignore"):
        q = [_clamp(c / m * F(255) + half, F(0), F(255)) for c in (x, y, z)] + [_clamp(F(255) * m / F(4) + half, F(1), F(255))]
    return np.stack([c.astype(np.uint8) for c in q], axis=-1)


def oracle_rgbm(levels, rules=CONTRACT):
    """levels: [level 0, ..., level 4] of float32 (6, s, s, 4) -> [face][level] of uint8 (s, s, 4), as saveCubemap's loop feeds the compressor"""
    return [[rgbm_texels(lv[face], rules) for lv in levels] for face in range(6)]


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def hdr_cubemaps(seed, n, S):
    """log-uniform colours in 1e-3 .. 1e4, alpha 1"""
    rng = np.random.default_rng(seed)
    a = np.ones((n, 6, S, S, 4), F)
    a[..., :3] = f32(10.0 ** rng.uniform(-3.0, 4.0, (n, 6, S, S, 3)))
    return a


def gradient_cubemaps(S):
    """two probes of different content: a smooth gradient, and the same plus one texel at 1e4; a subnormal and a negative channel in the first"""
    f, y, x = np.meshgrid(np.arange(6), np.arange(S), np.arange(S), indexing="ij")
    a = np.ones((2, 6, S, S, 4), F)
    a[0, ..., 0] = f32(0.1 + x / S)
    a[0, ..., 1] = f32(0.2 + y / S * 0.5)
    a[0, ..., 2] = f32(0.05 * (f + 1))
    a[1] = a[0]
    a[1, 2, S // 3, S // 2, :3] = 1e4
    a[0, 0, 0, 0, 0] = 1e-40  # a subnormal: kept, not flushed
    a[0, 0, 0, 1, 0] = 2e-45
    a[0, 5, 1, 1, 2] = -0.25
    a[0, 1, 2:4, 2:4, 3] = 3e-39  # a whole 2 x 2 block of subnormals: its average is one too
    return a


def rgbm_routes():
    """one cubemap (6, 16, 16, 4) whose texels take every route of saveCubemap's clamps: negative channels, m below 1 / 64 and above 4, rounding ties"""
    cm = np.ones((6, 16, 16, 4), F)
    vals = np.array([-1.0, -1e-3, 0.0, 1e-40, 1e-3, 1 / 64, 1 / 64 + 1e-4, 0.1, 0.5 / 255, 1.5 / 255 * 0.1, 1.0, 3.999, 4.0, 4.5, 100.0, 1e4], F)
    cm[:, :, :, 0] = vals[None, None, :]
    cm[:, :, :, 1] = vals[None, :, None]
    cm[..., 2] = np.array([-0.5, 0.0, 0.02, 0.3, 2.0, 7.0], F)[:, None, None]
    return cm


def cases():
    """name -> dict(cubemaps (n, 6, S, S, 4), mips: whether the mip chain applies). SH sizes 1, 2, 5, 16, 7 (294 pixels: one whole staging
    chunk of 256 and a part of one) and one probe of 128; batches of 1, 3 and 5."""
    return {
        "sh S=1 n=1": dict(cubemaps=hdr_cubemaps(1, 1, 1), mips=False),
        "sh S=2 n=3": dict(cubemaps=hdr_cubemaps(2, 3, 2), mips=False),
        "sh S=5 n=5": dict(cubemaps=hdr_cubemaps(3, 5, 5), mips=False),
        "sh S=7 n=3": dict(cubemaps=hdr_cubemaps(4, 3, 7), mips=False),
        "sh S=16 n=5": dict(cubemaps=hdr_cubemaps(5, 5, 16), mips=True),
        "sh S=128 n=1": dict(cubemaps=hdr_cubemaps(6, 1, 128), mips=False),
        "gradient S=16": dict(cubemaps=gradient_cubemaps(16), mips=True, filter=True),
        "gradient S=32": dict(cubemaps=gradient_cubemaps(32), mips=True, filter=True),
    }


def run_case(c, rules=CONTRACT):
    """-> dict(sh (n, 9, 3)[, mip1 ... (n, 6, s, s, 4)])"""
    cm = c["cubemaps"]
    r = dict(sh=np.stack([sh_compute(p, rules) for p in cm]))
    if c["mips"]:
        chains = [mip_chain(p, rules) for p in cm]
        for m in range(len(chains[0])):
            r[f"mip{m + 1}"] = np.stack([ch[m] for ch in chains])
    if c.get("filter"):
        levels = [filter_levels(p, rules) for p in cm]
        for k in range(5):
            r[f"level{k}"] = np.stack([lv[k] for lv in levels])
    return r
