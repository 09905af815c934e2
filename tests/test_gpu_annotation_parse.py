"""GPU: `dad3d_annotation_parse` (csrc/annotation_parse.hip) against the serial statement of its lifting rule
(tests/annotation_restatement.py): the status equal exactly, the values of a lifted document equal bitwise, a flagged document NaN in all
three outputs, and every document parsed as if it were alone."""
import itertools
import json

import numpy as np
import pytest
import torch

import annotation_restatement as R
from dad_3dheads_amd import _lib

pytestmark = pytest.mark.gpu
TILE = 4096
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def pack(docs):
    table, at = [], 0
    for doc in docs:
        table.append((at, len(doc)))
        at += (len(doc) + 15) // 16 * 16
    buf = np.zeros(max(at, 16), dtype=np.uint8)
    for (off, size), doc in zip(table, docs):
        buf[off:off + size] = np.frombuffer(doc, dtype=np.uint8)
    return buf, np.array(table, dtype=np.int64).reshape(-1, 2)


def launch(lib, buf, table, n_verts):
    """(status, vertices, model_view, projection) as numpy; the outputs are filled with a sentinel first, so nothing stays unwritten."""
    b = len(table)
    text = torch.from_numpy(buf).cuda()
    offsets, sizes = torch.from_numpy(table[:, 0].copy()).cuda(), torch.from_numpy(table[:, 1].copy()).cuda()
    v = torch.full((b, n_verts, 3), SENTINEL, dtype=torch.float32, device="cuda")
    m = torch.full((b, 4, 4), SENTINEL, dtype=torch.float32, device="cuda")
    p = torch.full((b, 4, 4), SENTINEL, dtype=torch.float32, device="cuda")
    status = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.dad3d_annotation_parse(text.data_ptr(), text.numel(), offsets.data_ptr(), sizes.data_ptr(), b, n_verts, v.data_ptr(),
                                          m.data_ptr(), p.data_ptr(), status.data_ptr(), 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status.cpu().numpy(), v.cpu().numpy(), m.cpu().numpy(), p.cpu().numpy()


def parse(lib, docs, n_verts):
    return launch(lib, *pack(docs), n_verts)


def check(lib, docs, n_verts, names=None):
    """One launch over `docs`; every item against the restatement. Returns the statuses."""
    status, v, m, p = parse(lib, docs, n_verts)
    for i, doc in enumerate(docs):
        tag = (names[i] if names else i, doc[:60])
        want, rv, rm, rp = R.restate(doc, n_verts, lib)
        assert status[i] == want, (tag, hex(status[i]), hex(want))
        if want == 0:
            assert v[i].tobytes() == rv.tobytes() and m[i].tobytes() == rm.tobytes() and p[i].tobytes() == rp.tobytes(), tag
        else:
            assert np.isnan(v[i]).all() and np.isnan(m[i]).all() and np.isnan(p[i]).all(), tag
    return status


def good(n_verts=2, head="", tail="", v=None, m=None, p=None):
    bv, bm, bp = R.base_parts(n_verts)
    return ('{%s"vertices":%s,"model_view_matrix":%s,"projection_matrix":%s%s}' % (head, v or bv, m or bm, p or bp, tail)).encode()


def padded_to(doc, length):
    """`doc` with spaces behind its opening brace, `length` bytes long."""
    assert doc[:1] == b"{" and length >= len(doc)
    return b"{" + b" " * (length - len(doc)) + doc[1:]


def straddling(doc, piece, line=TILE):
    """For every split of `piece` (its first appearance in `doc`): the document padded so that the split falls on byte `line`."""
    at = doc.index(piece)
    assert at > 0
    return [padded_to(doc, len(doc) + line - j - at) for j in range(1, len(piece))]


def test_document_lengths(lib):
    doc = good()
    docs = [b"", b"{", b" ", doc] + [padded_to(doc, n) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE + 5, 5 * TILE - 16)]
    status = check(lib, docs, 2)
    assert status[:3].all() and not status[3:].any()


def test_tokens_across_the_tile_line(lib):
    number, key = b"0.12345678901234567", b'"model_view_matrix"'
    doc = good(m="[[1,0,0,0],[0,1,0,0],[0,0,1,0],[0.12345678901234567,-0.5,2,1]]", tail=',"q":"a\\"b","r":"c\\\\","s":"\\\\\\"x"')
    docs = []
    for piece in (number, key, b'"a\\"b"', b'"c\\\\",', b'"\\\\\\"x"', b"],[", b'"vertices":', b"3e-2]],"):
        docs += straddling(doc, piece)
        docs += straddling(doc, piece, 2 * TILE)[:3]
    status = check(lib, docs, 2)
    assert not status.any()
    # the same splits in broken documents: an odd quote, and a number the routine flags, on either side of the line
    broken = doc.replace(b'"a\\"b"', b'"a\\\\"b"')
    assert check(lib, straddling(broken, b'"a\\\\"b"'), 2).all()
    digits = doc.replace(number, b"0.12345678901234567891")
    assert (check(lib, straddling(digits, b"0.12345678901234567891"), 2) == R.NUMBER).all()


def test_key_orders_and_extra_keys(lib):
    rng = np.random.default_rng(2)
    plain = [e for e in R.EXTRAS if not isinstance(e[1], dict)]
    docs = []
    for order in itertools.permutations(range(3)):
        docs.append(R.document(rng, 7, order=order))
        for places in ((2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 1), (3, 3, 3)):
            docs.append(R.document(rng, 7, kind="mixed", order=order, extras=plain, places=places, separators=(",", ":")))
    assert not check(lib, docs, 7).any()


def test_strings_nested_arrays_and_layouts(lib):
    rng = np.random.default_rng(3)
    tricky = [("brackets", ']]}{[[ , : "vertices": [[1,2,3]]'), ("vertices ", "x"), ("nested", [1, [2.5, [3e5, [-4, ["five", [], [[]]]]]]]),
              ("model_view_matrix2", [[1, 2], [3]]), ("t", True), ("f", False), ("n", None), ("esc", 'q"q\\q/q\bq\fq\nq\rq\tq')]
    docs = [R.document(rng, 7, extras=tricky, places=(3, 2, 2), separators=(",", ":")),
            R.document(rng, 7, extras=tricky, places=(0, 4, 0), indent=4),
            R.document(rng, 7, extras=tricky, places=(1, 1, 1), indent=4).replace(b"\n", b"\r\n"),
            R.document(rng, 7, extras=tricky, places=(8, 0, 0), indent=0).replace(b"\n", b"\t\n "),
            R.document(rng, 7, kind="double", sort_keys=True, extras=tricky, indent=2)]
    assert not check(lib, docs, 7).any()


@pytest.mark.parametrize("n_verts", [2, 7])
def test_bad_documents_are_flagged_as_the_rule_says(lib, n_verts):
    bad = R.bad_documents(n_verts)
    status = check(lib, list(bad.values()), n_verts, list(bad))
    assert status.all()
    by_name = dict(zip(bad, status))
    for name, flag in (("duplicate key", R.KEYS), ("duplicate extra key", R.KEYS), ("long key", R.KEYS), ("too many keys", R.KEYS),
                       ("nested object", R.GRAMMAR), ("one row fewer", R.SHAPE), ("one row more", R.SHAPE),
                       ("row of 2", R.SHAPE), ("row of 4", R.SHAPE), ("flat matrix", R.SHAPE), ("20 digits", R.NUMBER),
                       ("trailing comma in array", R.GRAMMAR), ("bare word", R.GRAMMAR), ("high byte", R.STRING)):
        assert by_name[name] == flag, name
    for name, flag in (("escaped key", R.KEYS), ("NaN", R.GRAMMAR), ("top-level array", R.GRAMMAR), ("truncated", R.GRAMMAR)):
        assert by_name[name] & flag, name


def test_long_backslash_runs_and_long_words(lib):
    docs = [good(tail=',"a":"' + "\\\\" * k + '"') for k in (1, 31, 32, 33, 40)]
    docs += [good(tail=',"a":"' + "\\\\" * k + '\\""') for k in (31, 32, 33)]
    docs += [good(tail=',"a":' + "0." + "0" * k + "1") for k in (28, 29, 30, 31)]
    docs += [good(tail=',"a' + "\\\\" * 3 + '":1')]
    status = check(lib, docs, 2)
    assert not status[:2].any() and status[4] and status[-1] & R.KEYS


def test_keys_at_the_limits_and_repeats_across_tiles(lib):
    many = "".join(',"k%d":%d' % (i, i) for i in range(125))  # 128 keys with the three names
    docs = [good(tail=many), good(tail=many + ',"one_more":1'), good(tail=',"' + "k" * 64 + '":1'), good(tail=',"' + "k" * 65 + '":1')]
    far = good(head='"id":1,', tail=',"pad":"' + "x" * 5000 + '","id":2')  # the repeat lies two tiles behind the first
    assert far.rindex(b'"id"') // TILE >= 1
    status = check(lib, docs + [far, far.replace(b'"id":2', b'"iD":2')], 2)
    assert status.tolist() == [0, R.KEYS, 0, R.KEYS, R.KEYS, 0]


def test_documents_are_parsed_in_isolation(lib):
    rng = np.random.default_rng(4)
    ok = [R.document(rng, 7, kind="mixed", indent=2, extras=R.EXTRAS[2:5]) for _ in range(3)]
    odd_quotes = ok[0].replace(b'"vertices"', b'"vertices', 1)
    unclosed = ok[1].replace(b"]", b" ", 1)[:-1]
    docs = [ok[0], odd_quotes, ok[1], unclosed, ok[2]]
    status, v, m, p = parse(lib, docs, 7)
    assert status.tolist()[0::2] == [0, 0, 0] and status[1] and status[3]
    for i in (1, 3):
        assert np.isnan(v[i]).all() and np.isnan(m[i]).all() and np.isnan(p[i]).all()
        assert status[i] == R.restate(docs[i], 7, lib)[0]
    for i in (0, 2, 4):
        alone = parse(lib, [docs[i]], 7)
        assert alone[0][0] == 0
        for got, one in zip((v, m, p), alone[1:]):
            assert got[i].tobytes() == one[0].tobytes()
        ref = R.load_mesh_of(docs[i])
        assert v[i].tobytes() == ref[0].tobytes() and m[i].tobytes() == ref[1].tobytes() and p[i].tobytes() == ref[2].tobytes()
    # the same five with zero bytes and garbage between them: the padding belongs to no document
    buf, table = pack(docs)
    for (off, size), nxt in zip(table[:-1], table[1:, 0]):
        buf[off + size:nxt] = 0x22
    again = launch(lib, buf, table, 7)
    assert np.array_equal(again[0], status) and again[1].tobytes() == v.tobytes()


def test_a_document_outside_the_buffer_is_not_read(lib):
    docs = [good(), good(), good(), good()]
    buf, table = pack(docs)
    table[1, 0] += 8  # not a multiple of 16
    table[2, 1] = buf.size  # runs past the end
    table[3, 0] = -16
    status, v, m, p = launch(lib, buf, table, 2)
    assert status.tolist() == [0, R.RANGE, R.RANGE, R.RANGE]
    assert np.isnan(v[1:]).all() and np.isnan(m[1:]).all() and np.isnan(p[1:]).all()
    assert v[0].tobytes() == R.load_mesh_of(docs[0])[0].tobytes()


@pytest.mark.parametrize("n_verts,count", [(1, 24), (7, 24), (85, 12), (5023, 1)])
def test_must_lift_sweep(lib, n_verts, count):
    docs = R.sweep(200 + n_verts, n_verts, count)
    status, v, m, p = parse(lib, docs, n_verts)
    assert not status.any(), status
    for i, doc in enumerate(docs):
        rv, rm, rp = R.load_mesh_of(doc)
        assert v[i].tobytes() == rv.tobytes() and m[i].tobytes() == rm.tobytes() and p[i].tobytes() == rp.tobytes(), i
        if n_verts <= 7 or i == 0:
            want, sv, _, _ = R.restate(doc, n_verts, lib)
            assert want == 0 and sv.tobytes() == rv.tobytes()


def test_wrong_vertex_count_and_special_numbers(lib):
    rng = np.random.default_rng(6)
    doc = R.document(rng, 7)
    assert check(lib, [doc], 6)[0] == R.SHAPE and check(lib, [doc], 8)[0] == R.SHAPE
    special = good(n_verts=3, v="[[16777217,-0.0,1e300],[-0,9007199254740992,-1e300],[0.1,1.0000000596046448,1e-46]]")
    status, v, _, _ = parse(lib, [special], 3)
    assert status[0] == 0
    with np.errstate(over="ignore"):
        assert v[0].tobytes() == np.array(json.loads(special)["vertices"], dtype=np.float32).tobytes()
    assert np.isinf(v[0, 0, 2]) and np.signbit(v[0, 0, 1]) and not np.signbit(v[0, 1, 0])
