"""The animation clip writer in numpy: ModelImporter::writeAnimations (renderer/editor/model_importer.cpp:1508-1754, helpers :34-146) from
all_keys to the last bit_writer.write, restated from the issue's contract and independent of csrc/lmx_animcomp.h. TEST INFRASTRUCTURE.

    compress(keys, bind, has_keys, translation_error, rotation_error, mutant) -> dict

keys: float32 (n_samples, n_bones, 7) = pos xyz, rot xyzw; bind: float32 (n_bones, 3). The dict has the fields of LmxAnimCompInfo, the four
tables in the library's dtypes (bone_index = the bone's place in the clip) and the two streams as uint8.

Where the reference is undefined the library's contract holds: a zero-range channel of an animated track packs the field 0; log2(u32(0))
is 0; a clip with a quotient of 2^32 or more, a channel above 30 bits, an entry above 57 bits or a frame above 65535 bits is refused (its
status says with what; the smallest code that applies), as is one without samples, with an error that is not finite and positive, a
non-finite key or a non-finite bind position of a bone with keys.

MUTANTS are one-rule changes; tests/test_animcomp_cpu.py shows that each changes a byte of some case."""
import numpy as np

F = np.float32
CONST_TRANSLATION = np.dtype([("value", "<f4", 3), ("bone_index", "<u2"), ("_pad", "<u2")], align=True)
TRANSLATION_TRACK = np.dtype([("min", "<f4", 3), ("to_range", "<f4", 3), ("offset_bits", "<u2"), ("bone_index", "<u2"), ("bitsizes", "u1", 3), ("_pad", "u1")], align=True)
CONST_ROTATION = np.dtype([("value", "<f4", 4), ("bone_index", "<u2"), ("_pad", "<u2")], align=True)
ROTATION_TRACK = np.dtype([("min", "<f4", 3), ("to_range", "<f4", 3), ("offset_bits", "<u2"), ("bone_index", "<u2"), ("bitsizes", "u1", 3), ("skipped_channel", "u1")], align=True)
OK, NO_SAMPLES, BAD_ERROR, NONFINITE_BIND, NONFINITE_KEY, QUOTIENT_RANGE, CHANNEL_BITS, ENTRY_BITS, FRAME_BITS = range(9)
TRANSLATION_STEP, ROTATION_STEP, BIND_ERROR = F(0.00005), F(0.000001), F(0.00001)
MUTANTS = ("tie_later", "no_half", "pack_fp32", "pow2", "clamp_from_1", "skip_last_largest", "sign_le", "bind_ge", "offsets_all_tracks")


def fold(column, later=False):
    """the sequential `p < min ? p : min` fold: on a tie the earlier sample's value stays (np.argmin / argmax return the first of equals, and
    -0.0 == +0.0)"""
    if later:
        return column[len(column) - 1 - np.argmin(column[::-1])], column[len(column) - 1 - np.argmax(column[::-1])]
    return column[np.argmin(column)], column[np.argmax(column)]


def range_bits(mn, mx, step, error):
    """(bits, refused)"""
    with np.errstate(all="ignore"):
        q = F(F(F(mx) - F(mn)) / step) / F(error)
    if not q < F(4294967296.0):
        return 0, True
    u = int(q)
    return (u.bit_length() - 1 if u else 0), False


def clamp(bits, first=0):
    bits = [max(b, 1) for b in bits]
    i = first
    while sum(bits) > 64:
        if bits[i] > 0:
            bits[i] -= 1
        i = (i + 1) % 4
    return bits


def to_range(mn, mx, bits, mutant=None):
    with np.errstate(all="ignore"):
        return F(F(mx) - F(mn)) / F((1 << bits) - (0 if mutant == "pow2" else 1))


def pack_field(v, mn, mx, bits, mutant=None):
    """one channel of every sample: v float32 (n_samples,) -> uint64 (n_samples,)"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        rng = F(F(mx) - F(mn))
        if rng == 0:
            return np.zeros(len(v), np.uint64)
        top = (1 << bits) - (0 if mutant == "pow2" else 1)
        d = v - F(mn)  # fp32
        if mutant == "pack_fp32":
            x = (d / rng * F(top) + F(0.5)).astype(np.float64)
        else:
            x = d.astype(np.float64) / np.float64(rng) * np.float64(top) + (0.0 if mutant == "no_half" else 0.5)
    return x.astype(np.uint64) & np.uint64((1 << bits) - 1)


def put(stream, at, value):
    byte, value = at >> 3, value << (at & 7)
    while value:
        stream[byte] |= value & 0xFF
        value >>= 8
        byte += 1


def compress(keys, bind, has_keys=None, translation_error=1.0, rotation_error=1.0, mutant=None):
    assert mutant is None or mutant in MUTANTS
    keys = np.ascontiguousarray(keys, F)
    ns, nb = keys.shape[:2]
    bind = np.ascontiguousarray(bind, F).reshape(nb, 3)
    has = np.ones(nb, bool) if has_keys is None else np.asarray(has_keys).astype(bool)
    te, re = F(translation_error), F(rotation_error)
    out = dict(n_const_translations=0, n_translations=0, n_const_rotations=0, n_rotations=0, translations_frame_size_bits=0, rotations_frame_size_bits=0,
               translation_stream_size=0, rotation_stream_size=0, frame_count=max(ns - 1, 0), status=OK)
    codes = []
    if ns == 0:
        codes.append(NO_SAMPLES)
    elif not (np.isfinite(te) and np.isfinite(re) and te > 0 and re > 0):
        codes.append(BAD_ERROR)
    ct, tt, cr, rt, t_entries, r_entries = [], [], [], [], [], []  # entries: (bone, offset, mins, maxs, bits, skipped)
    t_offset = r_offset = 0
    for b in range(nb if not codes else 0):
        if not has[b]:
            continue
        k = keys[:, b]
        if not np.isfinite(bind[b]).all():
            codes.append(NONFINITE_BIND)
        if not np.isfinite(k).all():
            codes.append(NONFINITE_KEY)
        if not (np.isfinite(bind[b]).all() and np.isfinite(k).all()):
            continue
        lo, hi = zip(*[fold(k[:, c], mutant == "tie_later") for c in range(7)])
        with np.errstate(all="ignore"):
            d = np.abs(k[:, :3] - bind[b][None, :])
        off_bind = (d >= BIND_ERROR).any() if mutant == "bind_ge" else (d > BIND_ERROR).any()
        if off_bind:
            bits, bad = zip(*[range_bits(lo[c], hi[c], TRANSLATION_STEP, te) for c in range(3)])
            if any(bad):
                codes.append(QUOTIENT_RANGE)
            if sum(bits) == 0:
                ct.append((k[0, :3], b))
            else:
                bits = [max(x, 1) for x in bits]
                if max(bits) > 30:
                    codes.append(CHANNEL_BITS)
                if sum(bits) > 57:
                    codes.append(ENTRY_BITS)
                tt.append((lo[:3], hi[:3], bits, t_offset, b))
                t_entries.append((b, t_offset, lo[:3], hi[:3], bits))
                t_offset += sum(bits)
            if mutant == "offsets_all_tracks" and sum(bits) == 0:
                t_offset += 3
        bits, bad = zip(*[range_bits(lo[3 + c], hi[3 + c], ROTATION_STEP, re) for c in range(4)])
        if any(bad):
            codes.append(QUOTIENT_RANGE)
        if sum(bits) == 0:
            cr.append((k[0, 3:], b))
            if mutant == "offsets_all_tracks":
                r_offset += 4
        else:
            bits = clamp(bits, 1 if mutant == "clamp_from_1" else 0)
            most = max(bits)
            skipped = (3 - bits[::-1].index(most)) if mutant == "skip_last_largest" else bits.index(most)
            if most > 30:
                codes.append(CHANNEL_BITS)
            entry = sum(bits) - most + 1
            if entry > 57:
                codes.append(ENTRY_BITS)
            rt.append((lo[3:], hi[3:], bits, r_offset, b, skipped))
            r_entries.append((b, r_offset, lo[3:], hi[3:], bits, skipped))
            r_offset += entry
    if not codes and (t_offset > 65535 or r_offset > 65535):
        codes.append(FRAME_BITS)
    if codes:
        out["status"] = min(codes)
        for name, dt in (("const_translations", CONST_TRANSLATION), ("translations", TRANSLATION_TRACK), ("const_rotations", CONST_ROTATION), ("rotations", ROTATION_TRACK)):
            out[name] = np.zeros(0, dt)
        out["translation_stream"] = out["rotation_stream"] = np.zeros(0, np.uint8)
        return out
    a = np.zeros(len(ct), CONST_TRANSLATION)
    for i, (v, b) in enumerate(ct):
        a[i]["value"], a[i]["bone_index"] = v, b
    out["const_translations"] = a
    a = np.zeros(len(tt), TRANSLATION_TRACK)
    for i, (lo, hi, bits, offset, b) in enumerate(tt):
        a[i]["min"], a[i]["to_range"] = lo, [to_range(lo[c], hi[c], bits[c], mutant) for c in range(3)]
        a[i]["bitsizes"], a[i]["offset_bits"], a[i]["bone_index"] = bits, offset, b
    out["translations"] = a
    a = np.zeros(len(cr), CONST_ROTATION)
    for i, (v, b) in enumerate(cr):
        a[i]["value"], a[i]["bone_index"] = v, b
    out["const_rotations"] = a
    a = np.zeros(len(rt), ROTATION_TRACK)
    for i, (lo, hi, bits, offset, b, skipped) in enumerate(rt):
        kept = [c for c in range(4) if c != skipped]
        a[i]["min"], a[i]["to_range"] = [lo[c] for c in kept], [to_range(lo[c], hi[c], bits[c], mutant) for c in kept]
        a[i]["bitsizes"], a[i]["offset_bits"], a[i]["bone_index"], a[i]["skipped_channel"] = [bits[c] for c in kept], offset, b, skipped
    out["rotations"] = a
    out.update(n_const_translations=len(ct), n_translations=len(tt), n_const_rotations=len(cr), n_rotations=len(rt), translations_frame_size_bits=t_offset,
               rotations_frame_size_bits=r_offset, translation_stream_size=(t_offset * ns + 7) // 8, rotation_stream_size=(r_offset * ns + 7) // 8)
    ts, rs = [0] * out["translation_stream_size"], [0] * out["rotation_stream_size"]
    for (b, offset, lo, hi, bits) in t_entries:
        v, shift = np.zeros(ns, np.uint64), 0
        for c in range(3):  # x in the low bits
            v |= pack_field(keys[:, b, c], lo[c], hi[c], bits[c], mutant) << np.uint64(shift)
            shift += bits[c]
        for s in range(ns):
            put(ts, t_offset * s + offset, int(v[s]))
    for (b, offset, lo, hi, bits, skipped) in r_entries:
        q = keys[:, b, 3:]
        v, shift = (q[:, skipped] <= 0 if mutant == "sign_le" else q[:, skipped] < 0).astype(np.uint64), 1
        for c in range(4):
            if c != skipped:
                v |= pack_field(q[:, c], lo[c], hi[c], bits[c], mutant) << np.uint64(shift)
                shift += bits[c]
        for s in range(ns):
            put(rs, r_offset * s + offset, int(v[s]))
    out["translation_stream"], out["rotation_stream"] = np.array(ts, np.uint8).reshape(-1), np.array(rs, np.uint8).reshape(-1)
    return out


TABLES = ("const_translations", "translations", "const_rotations", "rotations", "translation_stream", "rotation_stream")
FIELDS = ("n_const_translations", "n_translations", "n_const_rotations", "n_rotations", "translations_frame_size_bits", "rotations_frame_size_bits",
          "translation_stream_size", "rotation_stream_size", "frame_count", "status")


def flat(result):
    """every byte of a result in one array: the info's fields, the tables, the streams"""
    parts = [np.array([result[f] for f in FIELDS], np.uint64).view(np.uint8)]
    parts += [np.ascontiguousarray(result[t]).view(np.uint8).reshape(-1) for t in TABLES]
    return np.concatenate(parts)


def differences(got, want):
    """what differs between two results, for a message; empty when they are byte for byte the same"""
    bad = [f"{f}: {got[f]} vs {want[f]}" for f in FIELDS if int(got[f]) != int(want[f])]
    for t in TABLES:
        g, w = np.ascontiguousarray(got[t]).view(np.uint8).reshape(-1), np.ascontiguousarray(want[t]).view(np.uint8).reshape(-1)
        if g.size != w.size:
            bad.append(f"{t}: {g.size} vs {w.size} bytes")
        elif (g != w).any():
            at = np.flatnonzero(g != w)
            bad.append(f"{t}: {len(at)} of {g.size} bytes differ, first at {at[:4].tolist()}: {g[at[:4]].tolist()} vs {w[at[:4]].tolist()}")
    return bad


HEADER_MAGIC, VERSION_LAST, TRACK_CONSTANT, TRACK_ANIMATED = 0x5F4C4146, 8, 0, 1  # animation/animation.h:56-69


def ani_file(result, bone_hashes, skeleton_path, fps, root_motion_flags):
    """the .ani bytes write_animation leaves for a compressed clip (:1521-1736): header, the path and its zero, fps, samples - 1, flags, the
    translation count, its records as the bones come (constant and animated ones interleaved), the stream; the same for the rotations"""
    import struct

    out = struct.pack("<II", HEADER_MAGIC, VERSION_LAST) + skeleton_path.encode() + b"\0" + struct.pack("<fII", fps, result["frame_count"], root_motion_flags)
    for const, tracks, stream, rotation in ((result["const_translations"], result["translations"], result["translation_stream"], False),
                                            (result["const_rotations"], result["rotations"], result["rotation_stream"], True)):
        records = [(int(c["bone_index"]), struct.pack("<QB", int(bone_hashes[c["bone_index"]]), TRACK_CONSTANT) + c["value"].tobytes()) for c in const]
        for t in tracks:
            body = t["min"].tobytes() + t["to_range"].tobytes() + t["bitsizes"].tobytes() + struct.pack("<H", int(t["offset_bits"]))
            if rotation:
                body += struct.pack("<B", int(t["skipped_channel"]))
            records.append((int(t["bone_index"]), struct.pack("<QB", int(bone_hashes[t["bone_index"]]), TRACK_ANIMATED) + body))
        out += struct.pack("<I", len(records)) + b"".join(r for _, r in sorted(records, key=lambda r: r[0])) + np.ascontiguousarray(stream, np.uint8).tobytes()
    return out
