"""NumPy / Python restatement of the integer rule of csrc/obj_text.hip: the text `'%.8f' % float(np.float32(x))`
from 64-bit integer arithmetic only. Shared by tests/test_obj_text_host.py and tests/test_gpu_obj_text.py.

A float32 is (-1)^s m 2^e with m < 2^24 (e = E - 150, or -149 without the implicit bit when E = 0). P = m 10^8 < 2^51.
  e >= 0: Q = P << e, exact in 64 bits while e <= 13 (|x| < 2^37)
  e <  0: Q = P >> -e, rounded half to even on the shifted-out bits (0 when -e >= 64)
  text = '-' when the sign bit is set, Q // 10^8, '.', Q % 10^8 in eight digits
E = 255 or e > 13 is outside the domain: flagged, never text."""
import numpy as np

FLAG_NONFINITE, FLAG_LARGE = 1, 2
MAX_LINE_BYTES = 71
DOMAIN_LIMIT = 2.0 ** 37


def fixed8(x):
    """float32 array -> (Q uint64, sign bit, flag bits); Q is 0 where flagged."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    be = (u >> np.uint64(23)) & np.uint64(0xFF)
    frac = u & np.uint64(0x7FFFFF)
    m = np.where(be != 0, frac | np.uint64(0x800000), frac)
    e = np.where(be != 0, be.astype(np.int64) - 150, -149)
    flags = np.where(be == 255, FLAG_NONFINITE, np.where(e > 13, FLAG_LARGE, 0)).astype(np.int32)
    p = m * np.uint64(100000000)
    left = np.clip(e, 0, 13).astype(np.uint64)
    sh = np.clip(-e, 1, 63).astype(np.uint64)
    q_right = p >> sh
    rem = p & ((np.uint64(1) << sh) - np.uint64(1))
    half = np.uint64(1) << (sh - np.uint64(1))
    q_right = q_right + ((rem > half) | ((rem == half) & ((q_right & np.uint64(1)) == 1))).astype(np.uint64)
    q = np.where(e >= 0, p << left, np.where(-e >= 64, np.uint64(0), q_right))
    q = np.where(flags != 0, np.uint64(0), q)
    return q, (u >> np.uint64(31)).astype(bool), flags


def number_text(q, neg):
    q = int(q)
    return f"{'-' if neg else ''}{q // 100000000}.{q % 100000000:08d}"


def numbers(x):
    """float32 array -> list of str, None where the value is flagged."""
    q, neg, flags = fixed8(np.asarray(x, dtype=np.float32).reshape(-1))
    return [None if f else number_text(a, s) for a, s, f in zip(q.tolist(), neg.tolist(), flags.tolist())]


def vertex_block(vertices):
    """`vertices [N,3]` float32 -> (bytes of the N `v` lines, 0), or (None, flag bits) when a value is outside the domain."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    q, neg, flags = fixed8(v.reshape(-1))
    if flags.any():
        return None, int(np.bitwise_or.reduce(flags))
    t = [number_text(a, s) for a, s in zip(q.tolist(), neg.tolist())]
    return "".join(f"v {t[i]} {t[i + 1]} {t[i + 2]}\n" for i in range(0, len(t), 3)).encode("ascii"), 0


def python_numbers(x):
    """What the reference's `'%.8f' % value` prints for each float32."""
    return ["%.8f" % float(v) for v in np.asarray(x, dtype=np.float32).reshape(-1)]


def vertex_lines(obj_bytes):
    """The `v` lines (each with its newline) of the bytes of an .obj file."""
    return [line for line in bytes(obj_bytes).splitlines(keepends=True) if line.startswith(b"v ")]


def load_golden(path):
    """tests/golden/obj_text_golden.npz -> {name: (float32 vertices [N,3], bytes of the vertex block MeshSaver wrote)}."""
    out = {}
    with np.load(path) as z:
        for name in [str(n) for n in z["names"]]:
            out[name] = (z[f"vertices_{name}"], b"".join(vertex_lines(z[f"obj_{name}"].tobytes())))
    return out
