"""Python mirror of anim::Controller::update and the nodes of animation/nodes.cpp (the checker of lmx_animators_update): fp32 with one
rounding per operation (numpy float32 scalars), double where the reference uses double, recursive like the reference - not like the
library's explicit-stack VM. Pinned to the reference's own nodes.cpp by tests/test_controller_oracle_vs_ref.py.

A controller is a tree of tuples (tests/controller_cases.py writes the same tree as the compiled resource):
    ("anim", slot, flags)                                        ("blend1d", [(value, slot), ...], value)
    ("blend2d", [(x, y, slot), ...], [(a, b, c), ...], vx, vy)   ("select", blend_length, [children], value)
    ("switch", blend_length, true, false, value)                 ("playrate", value, child)
    ("ik", bones_count, leaf_hash, alpha, effector, child)
and a value is ("input", index), ("const", type, payload) or (op, v0, v1) with op one of MATH.
Runtime data is a list of u32 words (SwitchNode's RuntimeData word: current | switching << 8, its padding zero)."""
import math

import numpy as np

f32 = np.float32
ONE_SECOND = 1 << 15
NUMBER, BOOL, VEC3 = 0, 1, 2
MATH = ("eq", "neq", "lt", "gt", "lte", "gte", "mul", "div", "add", "sub", "and", "or")
COVERAGE = set()  # the branches the cases reached (filled by update)
LOOPED = 1


def bits(x):
    return int(np.array(x, f32).view(np.uint32))


def from_bits(u):
    return np.array(u & 0xFFFFFFFF, np.uint32).view(f32)[()]


def to_u32(x):
    """a float or double to u32 as the reference's x86-64 build converts it: through a 64-bit integer, low 32 bits; 0 for NaN / beyond +-2^63"""
    x = float(x)
    if math.isnan(x) or not (-9223372036854775808.0 <= x < 9223372036854775808.0):
        COVERAGE.add("u32_out_of_i64")
        return 0
    if not (0.0 <= x < 4294967296.0):
        COVERAGE.add("u32_wraps")
    return int(x) & 0xFFFFFFFF


def to_i32(x):
    x = float(x)
    if math.isnan(x) or not (-2147483648.0 <= x < 2147483648.0):
        COVERAGE.add("i32_indefinite")
        return -(1 << 31)
    return int(x)


def fmod1(x):
    return f32(math.fmod(float(x), 1.0))  # exact in any precision; carries x's sign (a zero too)


# ---- Time (animation.h:17-42, 180-183) ----
def seconds(v):
    return f32(v / float(ONE_SECOND))


def from_seconds(s):
    return to_u32(f32(s) * f32(ONE_SECOND))


def time_mul(v, t):
    return to_u32(f32(v) * f32(t))


def time_div(a, b):
    with np.errstate(all="ignore"):
        return f32(np.float64(a) / np.float64(b))


def time_lerp(a, b, t):
    return to_u32(float(a) * float(f32(1) - f32(t)) + float(b) * float(f32(t)))


# ---- core/math.cpp, scalar fp32 ----
def v_add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def v_mul(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def rotate(q, v):
    qv = (q[0], q[1], q[2])
    uv = cross(qv, v)
    uuv = cross(qv, uv)
    uv = v_mul(uv, f32(2) * q[3])
    uuv = v_mul(uuv, f32(2))
    return v_add(v_add(v, uv), uuv)


def qmul(a, r):
    return (a[3] * r[0] + r[3] * a[0] + a[1] * r[2] - r[1] * a[2], a[3] * r[1] + r[3] * a[1] + a[2] * r[0] - r[2] * a[0],
            a[3] * r[2] + r[3] * a[2] + a[0] * r[1] - r[0] * a[1], a[3] * r[3] - a[0] * r[0] - a[1] * r[1] - a[2] * r[2])


def lerp3(a, b, t):
    invt = f32(1) - t
    return tuple(a[k] * invt + b[k] * t for k in range(3))


def nlerp(q1, q2, t):
    inv = f32(1) - t
    if q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3] < 0:
        t = -t
    r = tuple(q1[k] * inv + q2[k] * t for k in range(4))
    l = f32(1) / np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3])
    return tuple(r[k] * l for k in range(4))


IDENTITY = ((f32(0), f32(0), f32(0)), (f32(0), f32(0), f32(0), f32(1)))


def rigid_mul(a, b):
    return (v_add(rotate(a[1], b[0]), a[0]), qmul(a[1], b[1]))


def rigid_inverted(a):
    rot = (a[1][0], a[1][1], a[1][2], -a[1][3])
    return (rotate(rot, (-a[0][0], -a[0][1], -a[0][2])), rot)


def interpolate(a, b, t):
    return (lerp3(a[0], b[0], t), nlerp(a[1], b[1], t))


def rigid_array(tr):
    return np.array(list(tr[0]) + list(tr[1]), f32)


# ---- Animation::getRootMotion (animation.cpp:272-291) and the two helpers of nodes.cpp:21-38 ----
def clip_root_motion(clip, time):
    pos, rot = IDENTITY
    frame = f32(time / float(ONE_SECOND) * float(clip["fps"]))
    idx = to_u32(frame)
    fc = clip["frame_count"]
    if idx < fc:
        frame_t = frame - f32(idx)
        if clip["rm_r"] is not None:
            rot = nlerp(tuple(clip["rm_r"][idx]), tuple(clip["rm_r"][idx + 1]), frame_t)
        if clip["rm_t"] is not None:
            pos = lerp3(tuple(clip["rm_t"][idx]), tuple(clip["rm_t"][idx + 1]), frame_t)
        return (pos, rot)
    COVERAGE.add("root_motion_back")
    if clip["rm_r"] is not None:
        rot = tuple(clip["rm_r"][fc])
    if clip["rm_t"] is not None:
        pos = tuple(clip["rm_t"][fc])
    return (pos, rot)


def root_motion_ex(clip, t0, t1):
    return rigid_mul(rigid_inverted(clip_root_motion(clip, t0)), clip_root_motion(clip, t1))


def root_motion_between(clip, t0_abs, t1_abs):
    length = clip["length"]
    t0, t1 = t0_abs % length, t1_abs % length
    if t0 <= t1:
        return root_motion_ex(clip, t0, t1)
    COVERAGE.add("root_motion_wraps")
    return rigid_mul(root_motion_ex(clip, t0, length), root_motion_ex(clip, 0, t1))


class Runtime:
    """anim::RuntimeContext of one Animator. `clips[slot]`: a clip dict or None; `bone_hashes`: the model's (for the IK record's leaf index)."""

    def __init__(self, tree, input_types, clips, bone_hashes=()):
        self.tree, self.input_types, self.clips, self.bone_hashes = tree, list(input_types), clips, list(bone_hashes)
        self.inputs = [(t, (0, 0, 0)) for t in self.input_types]  # (type, three words)
        self.weight = f32(1)
        self.root_motion = IDENTITY
        self.time_delta = 0
        self.blendstack = []
        self.data = []
        self.src, self.rd = [], 0
        self.enter(tree)  # Controller::createRuntime: enter with every input zero

    def set_input(self, idx, value):
        t = self.input_types[idx]
        if t == NUMBER:
            self.inputs[idx] = (t, (bits(value), 0, 0))
        elif t == BOOL:
            self.inputs[idx] = (t, (1 if value else 0, 0, 0))
        else:
            self.inputs[idx] = (t, tuple(bits(x) for x in value))

    # ---- ValueNode::eval: (type, words) ----
    def eval(self, v):
        if v[0] == "input":
            return self.inputs[v[1]]
        if v[0] == "const":
            t, p = v[1], v[2]
            return (t, (bits(p), 0, 0)) if t == NUMBER else (t, (1 if p else 0, 0, 0)) if t == BOOL else (t, tuple(bits(x) for x in p))
        a, b = self.eval(v[1]), self.eval(v[2])
        COVERAGE.add("math_" + v[0])
        if v[0] in ("and", "or"):
            assert a[0] == BOOL and b[0] == BOOL
            r = (a[1][0] != 0 and b[1][0] != 0) if v[0] == "and" else (a[1][0] != 0 or b[1][0] != 0)
            return (BOOL, (int(r), 0, 0))
        assert a[0] != BOOL and b[0] != BOOL  # .f of a BOOL
        x, y = from_bits(a[1][0]), from_bits(b[1][0])
        if np.isnan(x) or np.isnan(y):
            COVERAGE.add("math_nan_operand")
        with np.errstate(all="ignore"):
            if v[0] in ("mul", "div", "add", "sub"):
                if v[0] == "div" and y == 0:
                    COVERAGE.add("div_by_zero")
                r = {"mul": x * y, "div": x / y, "add": x + y, "sub": x - y}[v[0]]
                return (NUMBER, (bits(r), 0, 0))
        r = {"eq": x == y, "neq": x != y, "lt": x < y, "gt": x > y, "lte": x <= y, "gte": x >= y}[v[0]]
        return (BOOL, (int(bool(r)), 0, 0))

    def to_float(self, v):
        t, w = self.eval(v)
        assert t == NUMBER
        return from_bits(w[0])

    def child_index(self, v, n):
        i = to_i32(self.to_float(v) + f32(0.5))
        return min(max(i, 0), n - 1)

    def to_bool(self, v):
        t, w = self.eval(v)
        assert t == BOOL
        return w[0] != 0

    def read(self):
        self.rd += 1
        return self.src[self.rd - 1]

    # ---- enter / skip / update ----
    def enter(self, n):
        k = n[0]
        if k == "select":
            c = self.child_index(n[3], len(n[2]))
            self.data += [c, c, 0]
            self.enter(n[2][c])
        elif k == "switch":
            c = self.to_bool(n[4])
            self.data += [int(c), 0]
            self.enter(n[2] if c else n[3])
        elif k == "playrate":
            self.enter(n[2])
        elif k == "ik":
            self.enter(n[5])
        else:
            self.data.append(0)

    def skip(self, n):
        k = n[0]
        if k == "select":
            frm, to, _ = self.read(), self.read(), self.read()
            self.skip(n[2][frm])
            if frm != to:
                self.skip(n[2][to])
        elif k == "switch":
            d, _ = self.read(), self.read()
            current, switching = (d & 0xFF) != 0, (d & 0xFF00) != 0
            if switching:
                self.skip(n[3] if current else n[2])
            self.skip(n[2] if current else n[3])
        elif k == "playrate":
            self.skip(n[2])
        elif k == "ik":
            self.skip(n[5])
        else:
            self.read()

    def sample(self, slot, weight, time, looped):
        self.blendstack.append(("sample", slot, f32(weight), time, bool(looped)))

    def blend_children(self, tag, blend_length, t, frm, to):
        """the mid-transition part shared by SELECT and SWITCH (nodes.cpp:180-192, 280-292)"""
        COVERAGE.add(tag + "_mid_blend")
        if t == blend_length:
            COVERAGE.add(tag + "_t_equals_blend_length")
        self.update(frm)
        with np.errstate(all="ignore"):
            tq = seconds(t) / seconds(blend_length)
        if np.isnan(tq):
            COVERAGE.add("blend_weight_nan")
        lo = tq if tq > 0 else f32(0)  # clamp = minimum(maximum(t, 0), 1): NaN becomes 0
        tc = lo if lo < 1 else f32(1)
        old_w = self.weight
        self.weight = self.weight * tc
        tmp = self.root_motion
        self.update(to)
        self.weight = old_w
        self.root_motion = interpolate(tmp, self.root_motion, tq)

    def update(self, n):
        k = n[0]
        if k == "anim":
            t = self.read()
            prev_t = t
            t = (t + self.time_delta) & 0xFFFFFFFF
            if t < prev_t:
                COVERAGE.add("anim_time_wraps_32_bits")
            clip = self.clips[n[1]]
            looped = (n[2] & LOOPED) != 0
            COVERAGE.add("anim_looped" if looped else "anim_clamped")
            if clip is not None:
                if not looped:
                    if t > clip["length"]:
                        COVERAGE.add("anim_clamped_at_end")
                    t, prev_t = min(t, clip["length"]), min(prev_t, clip["length"])
                self.root_motion = root_motion_between(clip, prev_t, t)
                COVERAGE.add("clip_rm_%s%s" % ("t" if clip["rm_t"] is not None else "", "r" if clip["rm_r"] is not None else ""))
            else:
                self.root_motion = IDENTITY
            self.data.append(t)
            self.sample(n[1], self.weight, t, looped)
        elif k == "select":
            frm, to, t = self.read(), self.read(), self.read()
            child = self.child_index(n[3], len(n[2]))
            if frm != to:
                t = (t + self.time_delta) & 0xFFFFFFFF
                if child != to:
                    COVERAGE.add("select_choice_changed_mid_blend")
                if t > n[1]:
                    COVERAGE.add("select_blend_ends")
                    self.skip(n[2][frm])
                    self.data += [to, to, 0]
                    self.update(n[2][to])
                    return
                self.data += [frm, to, t]
                self.blend_children("select", n[1], t, n[2][frm], n[2][to])
                return
            if child != frm:
                COVERAGE.add("select_transition_start")
                self.data += [frm, child, 0]
                self.update(n[2][frm])
                self.enter(n[2][child])
                return
            COVERAGE.add("select_steady")
            self.data += [frm, to, (t + self.time_delta) & 0xFFFFFFFF]
            self.update(n[2][frm])
        elif k == "switch":
            d, t = self.read(), self.read()
            current, switching = (d & 0xFF) != 0, (d & 0xFF00) != 0
            cond = self.to_bool(n[4])
            tn, fn = n[2], n[3]
            if switching:
                t = (t + self.time_delta) & 0xFFFFFFFF
                if cond != current:
                    COVERAGE.add("switch_choice_changed_mid_blend")
                if t > n[1]:
                    COVERAGE.add("switch_blend_ends")
                    self.skip(fn if current else tn)
                    self.data += [int(current), 0]
                    self.update(tn if current else fn)
                    return
                self.data += [int(current) | 0x100, t]
                self.blend_children("switch", n[1], t, fn if current else tn, tn if current else fn)
                return
            if current != cond:
                COVERAGE.add("switch_transition_start")
                current = cond
                self.data += [int(current) | 0x100, 0]
                self.update(fn if current else tn)
                self.enter(tn if current else fn)
                return
            COVERAGE.add("switch_steady")
            self.data += [int(current), (t + self.time_delta) & 0xFFFFFFFF]
            self.update(tn if current else fn)
        elif k == "playrate":
            td = seconds(self.time_delta)
            v = self.to_float(n[1])
            rate = f32(0) if f32(0) > v else v  # maximum(0.f, v): a NaN rate stays
            COVERAGE.add("playrate_zero" if rate == 0 else "playrate_below_one" if rate < 1 else "playrate_above_one")
            if v < 0:
                COVERAGE.add("playrate_negative")
            if self.time_delta > (1 << 24):
                COVERAGE.add("playrate_time_delta_above_2_24")
            self.time_delta = time_mul(self.time_delta, rate)
            self.update(n[2])
            self.time_delta = from_seconds(td)
        elif k == "ik":
            self.update(n[5])
            alpha = self.to_float(n[3])
            if alpha > 0:
                COVERAGE.add("ik_alpha_clamped" if alpha > 1 else "ik_emitted")
                alpha = f32(1) if f32(1) < alpha else alpha
                t, w = self.eval(n[4])
                assert t == VEC3
                if n[4][0] == "input":
                    COVERAGE.add("ik_target_from_input")
                leaf = self.bone_hashes.index(n[2]) if n[2] in self.bone_hashes else 0xFFFFFFFF
                if leaf == 0xFFFFFFFF:
                    COVERAGE.add("ik_leaf_not_in_model")
                self.blendstack.append(("ik", alpha, tuple(from_bits(x) for x in w), leaf, n[1]))
            else:
                COVERAGE.add("ik_alpha_not_positive")
        elif k == "blend1d":
            relt = from_bits(self.read())
            relt0 = relt
            x = self.to_float(n[2])
            ch = n[1]
            a, b, pt = ch[0], None, f32(0)
            if x > f32(ch[0][0]):
                if x >= f32(ch[-1][0]):
                    COVERAGE.add("blend1d_at_or_above_last")
                    a = ch[-1]
                else:
                    for i in range(1, len(ch)):
                        if x < f32(ch[i][0]):
                            COVERAGE.add("blend1d_between")
                            pt = (x - f32(ch[i - 1][0])) / (f32(ch[i][0]) - f32(ch[i - 1][0]))
                            a, b = ch[i - 1], ch[i]
                            break
            else:
                COVERAGE.add("blend1d_on_first" if x == f32(ch[0][0]) else "blend1d_below_first")
            if len(ch) == 1:
                COVERAGE.add("blend1d_one_child")
            ca = self.clips[a[1]]
            cb = self.clips[b[1]] if b is not None else None
            if cb is not None:
                COVERAGE.add("blend1d_a_shorter" if ca["length"] < cb["length"] else "blend1d_a_longer")
            wlen = time_lerp(ca["length"], cb["length"] if cb is not None else ca["length"], pt)
            relt = fmod1(relt + time_div(self.time_delta, wlen))
            self.root_motion = root_motion_between(ca, time_mul(ca["length"], relt0), time_mul(ca["length"], relt))
            if cb is not None:
                tr1 = root_motion_between(cb, time_mul(cb["length"], relt0), time_mul(cb["length"], relt))
                self.root_motion = interpolate(self.root_motion, tr1, pt)
            self.data.append(bits(relt))
            self.sample(a[1], self.weight, time_mul(ca["length"], relt), True)
            if b is not None:
                self.sample(a[1], self.weight * pt, time_mul(cb["length"], relt), True)  # pair.a->slot, anim_b's length (nodes.cpp:681-687)
        elif k == "blend2d":
            relt = from_bits(self.read())
            relt0 = relt
            x, y = self.to_float(n[3]), self.to_float(n[4])
            ch = n[1]
            trio = None
            with np.errstate(all="ignore"):
                for (ia, ib, ic) in n[2]:
                    A, B, Cc = ch[ia], ch[ib], ch[ic]
                    abx, aby = f32(B[0]) - f32(A[0]), f32(B[1]) - f32(A[1])
                    acx, acy = f32(Cc[0]) - f32(A[0]), f32(Cc[1]) - f32(A[1])
                    apx, apy = x - f32(A[0]), y - f32(A[1])
                    d00, d01, d11 = abx * abx + aby * aby, abx * acx + aby * acy, acx * acx + acy * acy
                    d20, d21 = apx * abx + apy * aby, apx * acx + apy * acy
                    denom = d00 * d11 - d01 * d01
                    if denom == 0:
                        COVERAGE.add("blend2d_degenerate_triangle")
                    u = (d11 * d20 - d01 * d21) / denom
                    v = (d00 * d21 - d01 * d20) / denom
                    if u >= 0 and v >= 0 and u + v <= 1:
                        trio = (A[2], B[2], Cc[2], f32(1) - u - v, u, v)
                        COVERAGE.add("blend2d_on_edge" if (u == 0 or v == 0 or u + v == 1) else "blend2d_inside")
                        break
            if trio is None:
                COVERAGE.add("blend2d_outside_every_triangle")
                trio = (ch[0][2], ch[0][2], ch[0][2], f32(1), f32(0), f32(0))
            sa, sb, sc, ta, tb, tc = trio
            ca, cb, cc = self.clips[sa], self.clips[sb], self.clips[sc]
            if ca is None or cb is None or cc is None:
                COVERAGE.add("blend2d_empty_slot")
                self.data.append(bits(relt))
                return
            wlen = (time_mul(ca["length"], ta) + time_mul(cb["length"], tb) + time_mul(cc["length"], tc)) & 0xFFFFFFFF
            relt = fmod1(relt + time_div(self.time_delta, wlen))
            self.root_motion = root_motion_between(ca, time_mul(ca["length"], relt0), time_mul(ca["length"], relt))
            if tb > 0:
                tr1 = root_motion_between(cb, time_mul(cb["length"], relt0), time_mul(cb["length"], relt))
                self.root_motion = interpolate(self.root_motion, tr1, tb / (ta + tb))
            else:
                COVERAGE.add("blend2d_tb_zero")
            if tc > 0:
                tr1 = root_motion_between(cc, time_mul(cc["length"], relt0), time_mul(cc["length"], relt))
                self.root_motion = interpolate(self.root_motion, tr1, tc)
            else:
                COVERAGE.add("blend2d_tc_zero")
            self.data.append(bits(relt))
            self.sample(sa, self.weight, time_mul(ca["length"], relt), True)
            if tb > 0:
                self.sample(sb, self.weight * (tb / (ta + tb)), time_mul(cb["length"], relt), True)
            if tc > 0:
                self.sample(sc, self.weight * (tc / (ta + tb + tc)), time_mul(cc["length"], relt), True)
        else:
            raise ValueError(k)

    def frame(self, time_delta_seconds):
        """Controller::update with animator.ctx->time_delta = Time::fromSeconds(time_delta): (data words, blend stack, root motion)"""
        if time_delta_seconds == 0:
            COVERAGE.add("time_delta_zero")
        self.time_delta = from_seconds(f32(time_delta_seconds))
        self.src, self.rd = self.data, 0
        self.data = []
        self.blendstack = []
        self.update(self.tree)
        return list(self.data), list(self.blendstack), self.root_motion
