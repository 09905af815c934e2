"""The lifting rule of the device annotation reader (csrc/annotation_parse.hip, include/dad3d.h), stated as one serial
walk over the bytes of a document: `restate(doc, n_verts, lib)` -> (status, vertices, model_view, projection), the arrays only where the
status is 0. Every quantity is defined per byte, for any byte string, so a broken document has one status too. Shared by
tests/test_annotation_host.py and tests/test_gpu_annotation_parse.py, with the documents both sweep.

Status 0 requires all of the following; anything else sets a flag bit and the host's `json.load` reads the file.
  * Outside strings stand only space, tab, LF, CR, `{ } [ ] , :` and words: maximal runs of letters, digits and `+ - .`, at most
    MAX_WORD bytes long. A word that starts with a digit or `-` is a number token, which the number routine must not flag (NUMBER);
    any other word is `true`, `false` or `null` (GRAMMAR, as for any other byte).
  * A quote opens or closes a string unless an odd run of backslashes stands in front of it; runs are counted up to MAX_RUN and a longer
    one is flagged. A string byte is 0x20 .. 0x7E, and a backslash that is not itself escaped escapes one of `" \\ / b f n r t` (STRING).
  * The significant tokens are `{ } [ ] , :`, a string (at its opening quote) and a word. Each is legal given its kind, the two tokens in
    front of it and the depth in front of it: `{` only as the first token, nothing behind a `}`, `}` only at depth 1; at depth 1
    `"key" : value` separated by commas, at depth 2 and more values separated by commas. At the end quotes and brackets are balanced and
    the last token is `}` (GRAMMAR).
  * A key is a string at depth 1 behind `{` or `,`. "vertices", "model_view_matrix" and "projection_matrix" each appear exactly once, no
    key holds a backslash, and no key appears twice: keys are compared by the 32-bit FNV-1a hash of their bytes, so two keys with one
    hash count as a repeat; a key closes within MAX_KEY bytes and a document has at most MAX_KEYS keys (KEYS). The value of a key that
    is no repeat reaches from it to the next key.
  * In the value of "vertices": every number token at depth 3, no string or literal, no bracket deeper, every row of 3 numbers, n_verts
    rows; the matrices 4 rows of 4 (SHAPE).
A lifted number is `float(token)` or `int(token)` cast to float32 the way `np.array(list, dtype=np.float32)` casts.
"""
import json

import numpy as np

from json_parse_restatement import host_parse

GRAMMAR, KEYS, SHAPE, NUMBER, STRING, RANGE = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
MAX_RUN, MAX_WORD, MAX_KEY, MAX_KEYS = 64, 32, 64, 128
NONE, LBRACE, RBRACE, LBRACK, RBRACK, COMMA, COLON, STR, NUM, LIT = range(10)
_PUNCT = {ord("{"): LBRACE, ord("}"): RBRACE, ord("["): LBRACK, ord("]"): RBRACK, ord(","): COMMA, ord(":"): COLON}
_WS = set(b" \t\n\r")
_WORD = set(b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ+-.")
_ESCAPES = set(b'"\\/bfnrt')
_NAMES = {b'vertices"': 1, b'model_view_matrix"': 2, b'projection_matrix"': 3}


def _run(d, i):
    r = 0
    while r < MAX_RUN and i - 1 - r >= 0 and d[i - 1 - r] == 0x5C:
        r += 1
    return r


def _value_ended(p1, p2, depth):
    return p1 in (NUM, LIT, RBRACK) or (p1 == STR and (depth >= 2 or p2 == COLON))


def _legal(k, p1, p2, depth):
    if p1 == NONE:
        return k == LBRACE
    if p1 == RBRACE or k == LBRACE:
        return False
    if k == STR:
        return p1 in (LBRACE, COMMA, COLON) if depth == 1 else depth >= 2 and p1 in (LBRACK, COMMA)
    if k in (NUM, LIT, LBRACK):
        return p1 == COLON if depth == 1 else depth >= 2 and p1 in (LBRACK, COMMA)
    if k == COLON:
        return depth == 1 and p1 == STR and p2 in (LBRACE, COMMA)
    if k == COMMA:
        return depth >= 1 and _value_ended(p1, p2, depth)
    if k == RBRACK:
        return depth >= 2 and (p1 == LBRACK or _value_ended(p1, p2, depth))
    return depth == 1 and _value_ended(p1, p2, 1)  # RBRACE


def restate(doc, n_verts, lib):
    d, n = bytes(doc), len(doc)
    flags, in_string, depth, prev_word = 0, 0, 0, False
    p1 = p2 = NONE
    n_tok = nums = rows = 0
    key = None  # the last key: (token ordinal, numbers in front, rows in front)
    region, seen, done, hashes = 0, set(), set(), []
    numbers, stores = [], []  # every number token; (region, index, token) of the ones in place
    for i in range(n):
        c = d[i]
        quote = escaping = False
        if c in (0x22, 0x5C):
            run = _run(d, i)
            if run == MAX_RUN:
                flags |= STRING
            if run % 2 == 0:
                quote, escaping = c == 0x22, c == 0x5C
        code, word = NONE, False
        if quote:
            if not in_string:
                code = STR
            in_string ^= 1
        elif in_string:
            if c < 0x20 or c > 0x7E:
                flags |= STRING
            if escaping and (d[i + 1] if i + 1 < n else 0) not in _ESCAPES:
                flags |= STRING
            if c == 0x5C and key is not None and key[0] + 1 == n_tok:
                flags |= KEYS
        elif c in _PUNCT:
            code = _PUNCT[c]
        elif c in _WORD:
            word = True
            if not prev_word:
                code = NUM if (0x30 <= c <= 0x39 or c == 0x2D) else LIT
        elif c not in _WS:
            flags |= GRAMMAR
        prev_word = word
        if code == NONE:
            continue
        if not _legal(code, p1, p2, depth):
            flags |= GRAMMAR
        if code == STR and depth == 1 and p1 in (LBRACE, COMMA):
            name = next((v for k, v in _NAMES.items() if d[i + 1:i + 1 + len(k)] == k), 0)
            hashed, closed = 2166136261, False
            for j in range(MAX_KEY + 1):
                if i + 1 + j >= n:
                    break
                if d[i + 1 + j] == 0x22:
                    closed = True
                    break
                hashed = ((hashed ^ d[i + 1 + j]) * 16777619) & 0xFFFFFFFF
            again = (name != 0 and name in seen) or hashed in hashes  # keys are compared by their hash: unsure is flagged
            if again or not closed or len(hashes) >= MAX_KEYS:
                flags |= KEYS
            hashes.append(hashed)
            seen.add(name)
            key, region = (n_tok, nums, rows), 0 if again else name
        else:
            if region:
                nr, rr = nums - key[1], rows - key[2]
                width, height = (3, n_verts) if region == 1 else (4, 4)
                if depth == 1 and code in (STR, NUM, LIT):
                    flags |= SHAPE
                if depth >= 2 and code in (STR, LIT):
                    flags |= SHAPE
                if code == NUM and depth != 3:
                    flags |= SHAPE
                if code == LBRACK and depth >= 3:
                    flags |= SHAPE
                if code in (LBRACK, RBRACK) and depth == (2 if code == LBRACK else 3) and nr != width * rr:
                    flags |= SHAPE
                if code == RBRACK and depth >= 4:
                    flags |= SHAPE
                if code == RBRACK and depth == 2:
                    if rr == height and nr == width * height:
                        done.add(region)
                    else:
                        flags |= SHAPE
            if code in (NUM, LIT):
                end = i
                while end < n and end - i <= MAX_WORD and d[end] in _WORD:
                    end += 1
                if end - i > MAX_WORD:
                    flags |= GRAMMAR
                elif code == LIT:
                    if d[i:end] not in (b"true", b"false", b"null"):
                        flags |= GRAMMAR
                else:
                    numbers.append(d[i:end])
                    if region and depth == 3 and 0 <= nr < width * height:
                        stores.append((region, nr, d[i:end]))
        nums += code == NUM
        rows += code == LBRACK and depth == 2
        depth += (code in (LBRACE, LBRACK)) - (code in (RBRACE, RBRACK))
        p2, p1 = p1, code
        n_tok += 1
    if in_string or depth != 0 or p1 != RBRACE:
        flags |= GRAMMAR
    if not {1, 2, 3} <= seen:
        flags |= KEYS
    if done != {1, 2, 3}:
        flags |= SHAPE
    if numbers and host_parse(lib, [t.decode("ascii") for t in numbers])[2].any():
        flags |= NUMBER
    if flags:
        return flags, None, None, None
    out = {1: [None] * (n_verts * 3), 2: [None] * 16, 3: [None] * 16}
    for reg, at, tok in stores:
        assert out[reg][at] is None
        text = tok.decode("ascii")
        out[reg][at] = float(text) if any(ch in text for ch in ".eE") else int(text)
    with np.errstate(over="ignore"):
        arrays = [np.array(out[r], dtype=np.float32) for r in (1, 2, 3)]
    return 0, arrays[0].reshape(n_verts, 3), arrays[1].reshape(4, 4), arrays[2].reshape(4, 4)


def load_mesh_of(doc):
    """FlameDataset._load_mesh on the bytes of a file (text-mode `open` of an ASCII file decodes nothing away)."""
    data = json.loads(bytes(doc).decode("ascii"))
    with np.errstate(over="ignore"):
        return (np.ascontiguousarray(np.array(data["vertices"], dtype=np.float32).reshape(-1, 3)),
                np.ascontiguousarray(np.array(data["model_view_matrix"], dtype=np.float32).reshape(4, 4)),
                np.ascontiguousarray(np.array(data["projection_matrix"], dtype=np.float32).reshape(4, 4)))


# ---- documents -----------------------------------------------------------------------------------------------------------------------

def random_numbers(rng, count, kind):
    """`float32`: float32 values widened to double; `double`: arbitrary normal doubles (random bit patterns); `mixed`: those, ints (some
    beyond 2^24), -0.0, 1e300."""
    f32 = [float(x) for x in rng.standard_normal(count).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, count).astype(np.float32)]
    if kind == "float32":
        return f32
    bits = rng.integers(0, 2 ** 63, count, dtype=np.uint64) | (rng.integers(0, 2, count, dtype=np.uint64) << np.uint64(63))
    exp = (bits >> np.uint64(52)) & np.uint64(0x7FF)
    bits = np.where((exp == 0) | (exp == 0x7FF), bits ^ (np.uint64(0x3FF) << np.uint64(52)), bits)  # normal doubles only
    dbl = [float(x) for x in bits.view(np.float64)]
    if kind == "double":
        return dbl
    special = [0, 1, -1, 16777217, -33554435, 2 ** 53, -0.0, 0.0, 1e300, -1e300, 1e-300, 123456789012, 0.1, 1.5e-7]
    pick = rng.integers(0, 3, count)
    return [f32[i] if pick[i] == 0 else dbl[i] if pick[i] == 1 else special[int(rng.integers(len(special)))] for i in range(count)]


EXTRAS = [("bbox", [10, 20, 300, 400]), ("attributes", {"skip": 1}), ("name", 'a "quoted" \\ name\n{"vertices": [[1]]}'),
          ("flags", [True, False, None, "x", [1, [2.5, ["deep", []]]]]), ("score", -0.75), ("id", 12345678901234), ("none", None),
          ("brackets", "]]}{[[ , : \"vertices\": "), ("empty", ""), ("yes", True)]


def document(rng, n_verts, kind="float32", indent=None, separators=None, sort_keys=False, extras=(), order=(0, 1, 2), places=(0, 0, 0, 1)):
    """`json.dumps` of the three arrays in the key order `order`, with the extra (key, value) pairs spread `places` = how many in front,
    between the first and second, between the second and third; the rest behind. Extras that hold a dict are left out (a nested object
    is flagged)."""
    names = ["vertices", "model_view_matrix", "projection_matrix"]
    values = [np.array(random_numbers(rng, n_verts * 3, kind), dtype=object).reshape(n_verts, 3).tolist(),
              np.array(random_numbers(rng, 16, kind), dtype=object).reshape(4, 4).tolist(),
              np.array(random_numbers(rng, 16, kind), dtype=object).reshape(4, 4).tolist()]
    extras = [e for e in extras if not isinstance(e[1], dict)]
    items, at = [], 0
    for slot in range(3):
        items += extras[at:at + places[slot]]
        at += places[slot]
        items.append((names[order[slot]], values[order[slot]]))
    items += extras[at:]
    return json.dumps(dict(items), indent=indent, separators=separators, sort_keys=sort_keys).encode("ascii")


def sweep(seed, n_verts, count):
    """`count` must-lift documents at `n_verts`: every indent, both separators, both sort_keys, all three kinds of number, every key
    order, extras of the allowed kinds in every place."""
    import itertools

    rng = np.random.default_rng(seed)
    plain = [e for e in EXTRAS if not isinstance(e[1], dict)]
    orders = list(itertools.permutations(range(3)))
    docs = []
    for i in range(count):
        take = [plain[j] for j in rng.permutation(len(plain))[: int(rng.integers(0, len(plain) + 1))]]
        places = tuple(int(x) for x in rng.integers(0, 3, 3))
        indent = [None, 0, 2, 4][i % 4]
        separators = [None, (",", ":")][(i // 4) % 2]
        docs.append(document(rng, n_verts, kind=["float32", "double", "mixed"][i % 3], indent=indent, separators=separators,
                             sort_keys=bool((i // 8) % 2), extras=take, order=orders[i % 6], places=places))
    return docs


def base_parts(n_verts=2):
    """The three values as compact text with plain numbers, for hand-made documents."""
    v = "[" + ",".join("[%d.5,-%d,%de-2]" % (i, i + 1, i + 2) for i in range(n_verts)) + "]"
    m = "[[1,0,0,0],[0,1,0,0],[0,0,1,0],[0.25,-0.5,2,1]]"
    p = "[[2.5,0,0,0],[0,2.5,0,0],[0,0,-1.002,-1],[0,0,-0.2002,0]]"
    return v, m, p


def bad_documents(n_verts=2):
    """{name: bytes}: each must be flagged. `n_verts` rows are what the caller asks for."""
    v, m, p = base_parts(n_verts)
    vm1, vp1 = base_parts(n_verts - 1)[0], base_parts(n_verts + 1)[0]
    doc = lambda a=v, b=m, c=p, head="", tail="": ('{%s"vertices":%s,"model_view_matrix":%s,"projection_matrix":%s%s}' % (head, a, b, c, tail)).encode()  # noqa: E731
    flat = "[" + ",".join(str(i) for i in range(16)) + "]"
    good = doc()
    return {
        "duplicate key": doc(tail=',"vertices":' + v),
        "duplicate extra key": doc(head='"id":1,', tail=',"id":2'),
        "duplicate extra key, other value kinds": doc(tail=',"a":[1,2],"b":null,"a":"x"'),
        "long key": doc(tail=',"' + "k" * 65 + '":1'),
        "too many keys": doc(tail="".join(',"k%d":%d' % (i, i) for i in range(126))),
        "escaped key": good.replace(b'"vertices"', b'"vert\\u0069ces"'),
        "escaped extra key": doc(head='"a\\nb":1,'),
        "nested object": doc(tail=',"attributes":{"skip":1}'),
        "object in array": doc(tail=',"list":[{"a":1}]'),
        "one row fewer": doc(a=vm1),
        "one row more": doc(a=vp1),
        "row of 2": doc(a=v.replace(",%de-2]" % (n_verts + 1), "]")),
        "row of 4": doc(a=v.replace("[0.5,", "[0.5,7,")),
        "flat matrix": doc(b=flat),
        "matrix row of 3": doc(c=p.replace("[2.5,0,0,0]", "[2.5,0,0]")),
        "NaN": doc(a=v.replace("0.5", "NaN")),
        "-Infinity": doc(b=m.replace("0.25", "-Infinity")),
        "20 digits": doc(a=v.replace("0.5", "0.12345678901234567891")),
        "big int": doc(tail=',"id":9007199254740993'),
        "leading zero": doc(b=m.replace("0.25", "01")),
        "trailing comma in array": doc(a=v[:-1] + ",]"),
        "trailing comma in object": doc(tail=","),
        "doubled comma": doc(b=m.replace("],[", "],,[", 1)),
        "missing colon": good.replace(b'"model_view_matrix":', b'"model_view_matrix"'),
        "colon behind a value": doc(tail=',"a":"b":"c"'),
        "key without value": doc(tail=',"a"'),
        "bare word": doc(tail=',"a":nil'),
        "True": doc(tail=',"a":True'),
        "high byte": good[:-1] + b',"a":"caf\xc3\xa9"}',
        "control byte in string": doc(tail=',"a":"x\ty"'),
        "unicode escape": doc(tail=',"a":"\\u00e9"'),
        "bad escape": doc(tail=',"a":"\\x"'),
        "zero byte": good.replace(b",", b",\x00", 1),
        "top-level array": b"[" + good + b"]",
        "two documents": good + good,
        "text behind": good + b" 1",
        "truncated": good[: len(good) // 2],
        "truncated in string": good[:5],
        "odd quotes": good.replace(b'"vertices"', b'"vertices', 1),
        "unclosed bracket": doc(a=v[:-1]),
        "missing key": ('{"vertices":%s,"model_view_matrix":%s}' % (v, m)).encode(),
        "string for a matrix": doc(b='"x"'),
        "number in vertices at depth 2": doc(a="[1," + v[1:]),
        "string in vertices": doc(a=v.replace("0.5", '"0.5"')),
        "deeper vertices": doc(a=v.replace("[0.5,", "[[0.5],")),
        "empty": b"",
        "whitespace": b"  \n",
        "long word": doc(tail=',"a":' + "1" * 40),
        "backslash outside a string": good.replace(b",", b"\\,", 1),
    }
