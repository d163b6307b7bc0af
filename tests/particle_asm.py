"""A small assembler for the particle VM's byte stream: the layout of ParticleSystemResource::DataStream and InstructionType
(renderer/particle_system.h:72-122) as InputMemoryStream::read consumes it. The test programs are written with it; nothing of the
reference's particle scripts or their compiled bytecode is used.

    p = program(update=[add(CH(0), CH(0), SYS(TIME_DELTA))], emit=[mov(CH(0), LIT(0))], output=[mov(OUT(0), CH(0))])
"""
import struct

OPS = ["END", "ADD", "COS", "SIN", "NOISE", "SUB", "EMIT", "MUL", "MULTIPLY_ADD", "LT", "MOV", "RAND", "KILL", "SQRT", "GT", "MIX", "GRADIENT", "DIV", "SPLINE",
       "MESH", "MOD", "OR", "AND", "NOT", "BLEND", "MAX", "MIN", "CMP", "CMP_ELSE"]
OP = {n: i for i, n in enumerate(OPS)}
NONE, CHANNEL, SYSTEM_VALUE, OUTPUT, REGISTER, LITERAL, GLOBAL, ERROR = range(8)
TIME_DELTA, TOTAL_TIME, EMIT_INDEX, RIBBON_INDEX, ENTITY_X, ENTITY_Y, ENTITY_Z = range(7)
ARITY = {"COS": 1, "SIN": 1, "NOISE": 1, "SQRT": 1, "MOV": 1, "NOT": 1, "ADD": 2, "SUB": 2, "MUL": 2, "DIV": 2, "MOD": 2, "LT": 2, "GT": 2, "AND": 2, "OR": 2, "MAX": 2,
         "MIN": 2, "MULTIPLY_ADD": 3, "MIX": 3, "BLEND": 3}


def stream(kind, index=0, value=0.0):
    return struct.pack("<BBxxf", kind, index, value)


def CH(i): return stream(CHANNEL, i)
def REG(i): return stream(REGISTER, i)
def OUT(i): return stream(OUTPUT, i)
def SYS(i): return stream(SYSTEM_VALUE, i)
def GLOB(i): return stream(GLOBAL, i)
def LIT(v): return stream(LITERAL, 0, v)


def LIT_BITS(u):
    """a literal given by its bit pattern (NaN payloads, -0)"""
    return struct.pack("<BBxxI", LITERAL, 0, u)


def ins(name, dst, *src):
    assert len(src) == ARITY[name], name
    return bytes([OP[name]]) + dst + b"".join(src)


def _mk(name):
    return lambda dst, *src: ins(name, dst, *src)


add, sub, mul, div, mod, lt, gt, and_, or_, max_, min_ = (_mk(n) for n in ("ADD", "SUB", "MUL", "DIV", "MOD", "LT", "GT", "AND", "OR", "MAX", "MIN"))
cos, sin, noise, sqrt, mov, not_ = (_mk(n) for n in ("COS", "SIN", "NOISE", "SQRT", "MOV", "NOT"))
madd, mix, blend = (_mk(n) for n in ("MULTIPLY_ADD", "MIX", "BLEND"))
END = bytes([OP["END"]])
KILL = bytes([OP["KILL"]])


def rand(dst, lo, hi):
    return bytes([OP["RAND"]]) + dst + struct.pack("<ff", lo, hi)


def gradient(dst, src, keys, values):
    assert len(keys) == len(values)
    return bytes([OP["GRADIENT"]]) + dst + src + struct.pack("<I", len(keys)) + struct.pack(f"<{len(keys)}f", *keys) + struct.pack(f"<{len(values)}f", *values)


def block(body):
    """the bytes of a conditional block: its instructions and the END that closes it"""
    return b"".join(body) + END


def cmp(cond, body):
    b = block(body)
    return bytes([OP["CMP"]]) + cond + struct.pack("<H", len(b)) + b


def cmp_else(cond, true_body, false_body):
    t, f = block(true_body), block(false_body)
    return bytes([OP["CMP_ELSE"]]) + cond + struct.pack("<HH", len(t), len(f)) + t + f


def emit(target, body):
    return bytes([OP["EMIT"]]) + struct.pack("<I", target) + block(body)


def mesh(dst, index, sub): return bytes([OP["MESH"]]) + dst + index + bytes([sub])
def spline(dst, src, sub): return bytes([OP["SPLINE"]]) + dst + src + bytes([sub])


class Program:
    """The stream of one emitter and what ParticleSystemResource::Emitter keeps next to it."""

    def __init__(self, update=(), emit=(), output=(), channels=1, registers=0, outputs=1, emit_inputs=0, init_emit_count=0, emit_per_second=0.0):
        u, e, o = block(update), block(emit), block(output)
        self.bytes = u + e + o
        self.emit_offset, self.output_offset = len(u), len(u) + len(e)
        self.channels, self.registers, self.outputs, self.emit_inputs = channels, registers, outputs, emit_inputs
        self.init_emit_count, self.emit_per_second = init_emit_count, float(emit_per_second)

    def set_on(self, ps, system, emitter):
        ps.setProgram(system, emitter, self.bytes, self.emit_offset, self.output_offset, self.channels, self.registers, self.outputs, self.emit_inputs,
                      self.init_emit_count, self.emit_per_second)
