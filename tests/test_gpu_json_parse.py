"""GPU: the device JSON reader (csrc/json_parse.hip, dad_3dheads_amd/json_reader.py) against `json.loads` itself: the tree is equal
(`json.dumps` of both, which tells an int from a float and -0.0 from 0.0), and the set of lifted arrays, their shapes and their float64
bits are what a walk over `json.loads(text)` predicts (tests/json_parse_restatement.py). A document the reader could only parse by
falling back to the host would lift nothing, so every case that expects lifted arrays also proves the kernels ran."""
import json

import numpy as np
import pytest
import torch

import eval_restatement as er
import json_parse_restatement as P
from dad_3dheads_amd import _lib, benchmark_export, evaluation, json_reader

pytestmark = pytest.mark.gpu
TILE = _lib.JSON_PARSE_TILE_BYTES


def check(text, min_count=32, expect=None):
    """load(text) == json.loads(text), and lifts what the walk predicts (`expect`: that many arrays)."""
    data = text.encode("utf-8") if isinstance(text, str) else text
    want = json.loads(data)
    doc = json_reader.load(data, device=0, min_count=min_count)
    assert json.dumps(doc.to_python()) == json.dumps(want)
    predicted = P.predict_lifted(want, min_count)
    got = P.lifted_of(doc)
    assert [g[0] for g in got] == [p[0] for p in predicted]
    assert got == predicted
    if expect is not None:
        assert len(got) == expect, [g[0] for g in got]
    for r, a in zip(doc.records.tolist(), doc.arrays):  # the record's span is the array's own text
        assert data[r[0]:r[0] + 1] == b"[" and data[r[1] - 1:r[1]] == b"]" and json.loads(data[r[0]:r[1]]) == a.tolist()
    return doc


def seeded_tree(seed=3):
    rng = np.random.default_rng(seed)
    f32 = lambda *s: (rng.standard_normal(s) * 10.0 ** rng.integers(-5, 6, s)).astype(np.float32).astype(np.float64)  # noqa: E731
    return {
        "floats": f32(50).tolist(),
        "matrix": f32(20, 3).tolist(),
        "ints": rng.integers(-1000, 1000, 40).tolist(),
        "mixed": [int(v) if i % 3 == 0 else float(v) for i, v in enumerate(f32(45).round(2))],
        "doubles": (rng.uniform(1, 10, 64) * 10.0 ** rng.integers(-300, 300, 64)).tolist(),
        "zeros": [0, -0.0, 0.0, 1e5, 1e-05] * 8,
        "short": [1.5, 2.5, 3.5],
        "nested": {"inner": [{"row": f32(33).tolist(), "name": "x"}, {"row": f32(4, 8).tolist()}], "flag": True, "none": None},
        "scalar": 3.25, "text": "plain",
    }


@pytest.mark.parametrize("style", ["default", "indent", "compact", "tabs_crlf"])
def test_formattings_of_one_tree(style):
    tree = seeded_tree()
    text = {"default": json.dumps(tree), "indent": json.dumps(tree, indent=1), "compact": json.dumps(tree, separators=(",", ":")),
            "tabs_crlf": json.dumps(tree, indent="\t").replace("\n", "\r\n")}[style]
    doc = check(text, expect=8)
    assert doc.root["short"] == [1.5, 2.5, 3.5] and isinstance(doc.root["floats"], json_reader.DeviceArray)
    assert doc.root["matrix"].shape == (20, 3) and doc.root["nested"]["inner"][1]["row"].shape == (4, 8)
    a = doc.root["mixed"]
    assert torch.equal(a.tensor().cpu(), torch.tensor(tree["mixed"], dtype=torch.float64)) and a.tolist() == tree["mixed"]
    assert [type(v) for v in a.tolist()] == [type(v) for v in tree["mixed"]]
    assert np.array_equal(np.asarray(a, dtype=np.float32), np.asarray(tree["mixed"], dtype=np.float32))
    assert np.array_equal(a.float32().cpu().numpy(), np.asarray(tree["mixed"], dtype=np.float32))


def evaluator_shaped(seed=9, items=3, n=40):
    """A ground-truth list and a submission dict with the fields of eval_restatement.golden_json, from seeded values."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32).astype(np.float64).tolist()  # noqa: E731
    gt = [{"id": str(i), "vertices": f(n, 3), "model_view_matrix": f(4, 4), "projection_matrix": f(4, 4), "bbox": [3, 4, 200, 210],
           "image_height": 256, "attributes": {"pose": "front", "occlusions": False}} for i in range(items)]
    sub = {str(i): {"68_landmarks_2d": rng.integers(0, 256, (68, 2)).astype(np.float64).tolist(), "N_landmarks_3d": f(n, 3),
                    "rotation_matrix": f(3, 3), "7_landmarks_3d": f(7, 3)} for i in range(items)}
    return gt, sub


def test_evaluator_shaped_documents():
    gt, sub = evaluator_shaped()
    doc = check(json.dumps(gt), expect=3)
    assert [a.shape for a in doc.arrays] == [(40, 3)] * 3 and doc.root[1]["model_view_matrix"] == gt[1]["model_view_matrix"]
    doc = check(json.dumps(sub), expect=6)
    assert doc.root["2"]["68_landmarks_2d"].shape == (68, 2) and doc.root["2"]["N_landmarks_3d"].shape == (40, 3)
    check(json.dumps(sub), min_count=1, expect=12)  # the 3 x 3 and 7 x 3 fields too


def test_root_array_and_scalars():
    rng = np.random.default_rng(1)
    doc = check(json.dumps(rng.standard_normal(100).tolist()), expect=1)
    assert isinstance(doc.root, json_reader.DeviceArray) and doc.root.offset == 0
    check(" " + json.dumps(rng.standard_normal((50, 2)).tolist()) + "\n", expect=1)
    check("7", expect=0)
    check("[1,2,3]", min_count=2, expect=1)  # shorter than one wave
    check('"[1,2,3]"', min_count=1, expect=0)


def test_strings_are_opaque():
    nums = list(range(40))
    tree = {
        "[1,2]": "[3,4,5]", "digits 123": "4.5e6", 'q"uote': 'a"b', "back\\slash": "c\\", "ends in backslash\\": nums,
        "two\\\\": "\\\\", 'esc\\"': ['\\"', "[", nums, "]", '"'], "utf8 é ü 漢": "ключ [1,2,3]", "after": [float(v) for v in nums],
        "[" * 5: "]" * 7, "ctrl": "\t\n\r", "{": "}", "tail": nums,
    }
    for text in (json.dumps(tree), json.dumps(tree, ensure_ascii=False), json.dumps(tree, indent=2, ensure_ascii=False)):
        doc = check(text, expect=4)
        assert doc.root['esc\\"'][2].tolist() == nums
    check(json.dumps({"k": nums, "s": '[' + ",".join(map(str, nums)) + ']'}), expect=1)  # the same bytes inside a string stay text


def test_what_is_not_a_regular_array_of_numbers_stays_on_the_host():
    n40 = ",".join(str(i) for i in range(40))
    cases = {  # text -> lifted arrays
        "[%s,true]" % n40: 0, "[%s,null]" % n40: 0, "[%s,NaN]" % n40: 0, "[-Infinity,%s]" % n40: 0, "[Infinity,%s]" % n40: 0,
        '[%s,{"a":1}]' % n40: 0, '[%s,"x"]' % n40: 0, "[]": 0, "[[],[]]": 0, "[[%s],[]]" % n40: 0, "[[%s],[1,2]]" % n40: 0,
        "[[[%s]]]" % n40: 0, "[[[%s]],[[%s]]]" % (n40, n40): 0, "[1,[%s]]" % n40: 0, "[[%s],1]" % n40: 0, "[%s,[]]" % n40: 0,
        "[[1,[],2],[3],%s]" % ",".join("[%d]" % i for i in range(40)): 0,
        "[[%s],[%s]]" % (n40, n40): 1, '{"a":[[%s],[%s]],"b":[%s,true]}' % (n40, n40, n40): 1,
        '[[%s],[%s],"s"]' % (n40, n40): 2, '[{"a":[%s]},[%s]]' % (n40, n40): 2, "[[%s , %s ] ]" % (n40, n40): 1,
    }
    for text, lifted in cases.items():
        check(text, expect=lifted)
        check(" \n" + text.replace(",", " ,\t") + "\r\n", expect=lifted)


@pytest.mark.parametrize("token", ["12345678901234567890", "1.2345678901234567890123", "9007199254740993", "-9007199254740993", "5e-324",
                                   "2.2250738585072011e-308", "1e-400", "1e309", "1e400", "123456789012345678901234567890"])
def test_a_flagged_token_keeps_its_array_on_the_host(token):
    n40 = ",".join("%d.5" % i for i in range(40))
    text = '{"clean":[%s],"flagged":[%s,%s,%s],"rows":[[%s],[%s,%s]]}' % (n40, n40, token, n40, n40, n40, token)
    data = text.encode()
    doc = json_reader.load(data, device=0)
    want = json.loads(data)
    assert json.dumps(doc.to_python()) == json.dumps(want)
    assert [a.shape for a in doc.arrays] == [(40,)] and isinstance(doc.root["flagged"], list) and doc.root["flagged"] == want["flagged"]
    # 19 digits and integers up to 2^53 stay on the device
    ok = '{"a":[%s,123456789012345678.5,0.000001234567890123456789,9007199254740992,-9007199254740992,2.2250738585072014e-308,1.7976931348623157e308]}' % n40
    check(ok, expect=1)


def feature_document():
    """A 40-number array between strings that hold an escaped quote, brackets, UTF-8 and runs of backslashes (odd in front of an
    escaped quote, even in front of the closing one)."""
    numbers = [round(0.5 * i - 7, 1) if i % 2 else i - 20 for i in range(40)]
    tree = {'q"[1,2]\\': "é\\\\", "a": numbers, "b": '\\\\\\"' + "\\" * 6, "c": [1, 2]}
    return json.dumps(tree, ensure_ascii=False), numbers


def test_every_feature_slides_across_a_tile_edge():
    text, numbers = feature_document()
    data = text.encode("utf-8")
    want = json.dumps(json.loads(data))
    assert len(data) < 400 and b'\\\\\\\\\\\\\\"' in data and b'\\\\"' in data
    sizes = set()
    # every byte of the document, so every token, string, quote and backslash run, sits on either side of the first and second edge
    for edge in (TILE, 2 * TILE):
        for k in range(edge - len(data) - 2, edge + 3):
            doc = json_reader.load(b" " * k + data, device=0)
            assert json.dumps(doc.to_python()) == want, k
            assert [a.shape for a in doc.arrays] == [(40,)] and doc.arrays[0].tolist() == numbers, k
            assert doc.records[0, 0] == k + data.index(b"[-20") and doc.records[0, 1] == k + data.index(b', "b"'), k
            sizes.add(k + len(data))
    assert {TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1} <= sizes  # documents that end on, before and behind an edge


def test_document_sizes_around_a_tile():
    for size in (TILE - 1, TILE, TILE + 1, 3 * TILE):
        body = ",".join("%d" % (i % 10) for i in range(size))[:size - 2]
        body = body[:-1] if body.endswith(",") else body
        text = "[" + body + "]" + " " * (size - 2 - len(body))
        assert len(text) == size
        doc = check(text, expect=1)
        assert doc.records[0, 1] == len(body) + 2
    # a string that runs over several tiles, and a backslash run longer than a tile in front of the closing quote
    long = json.dumps({"s": "x" * (2 * TILE) + '"', "b": "\\" * (TILE + 3), "a": list(range(50)), "odd": "\\" * TILE + '"', "z": list(range(60))})
    check(long, expect=2)
    # ~1 MB
    rng = np.random.default_rng(5)
    big = {"v": rng.standard_normal((20000, 3)).astype(np.float32).astype(np.float64).tolist(), "w": rng.standard_normal(5000).tolist()}
    check(json.dumps(big), expect=2)


@pytest.mark.parametrize("text", [
    '{"a": [' + ",".join(map(str, range(50))),
    '{"a": [' + ",".join(map(str, range(50))) + ",]}",
    '{"a": [1 2,' + ",".join(map(str, range(50))) + "]}",
    '{"a": [' + ",".join(map(str, range(50))) + ",,7]}",
    '{"a": [' + ",".join(map(str, range(50))) + "] ]}",
    "[" + ",".join(map(str, range(50))) + "] 5",
    '{"a": [01,' + ",".join(map(str, range(50))) + "]}",
    '{"a": "unterminated [' + ",".join(map(str, range(50))) + "]",
    "",
], ids=["unclosed", "trailing_comma", "missing_comma", "double_comma", "extra_close", "extra_data", "leading_zero", "open_string", "empty"])
def test_malformed_documents_raise(text):
    with pytest.raises(json.JSONDecodeError):
        json.loads(text)
    with pytest.raises(json.JSONDecodeError):
        json_reader.load(text.encode(), device=0)


def test_placeholder_key_in_the_document_goes_to_the_host():
    tree = {json_reader.PLACEHOLDER_KEY: 0, "a": list(range(50))}
    doc = json_reader.load(json.dumps(tree).encode(), device=0)
    assert doc.root == tree and doc.arrays == [] and doc.values.numel() == 0


def test_load_reads_a_file(tmp_path):
    tree = seeded_tree(4)
    path = tmp_path / "doc.json"
    path.write_text(json.dumps(tree))
    doc = json_reader.load(str(path), device=0)
    assert json.dumps(doc.to_python()) == json.dumps(tree) and len(doc.arrays) == 8
    assert doc.values.dtype == torch.float64 and doc.is_int.dtype == torch.uint8 and doc.values.is_cuda


def _index(text_dev, n, lib):
    scratch_bytes = lib.dad3d_json_parse_scratch_bytes(n)
    scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    counts = torch.full((6,), -77, dtype=torch.int32, device="cuda")
    _lib.check(lib.dad3d_json_parse_index(text_dev.data_ptr(), n, scratch.data_ptr(), scratch_bytes, counts.data_ptr(), 0, None))
    return scratch, scratch_bytes, counts


def test_c_abi_writes_nothing_behind_the_counts():
    lib = _lib.load()
    text = ' {"k": "[9,9]", "a": [[1, 2.5], [3, -4e2]], "b": [10, 20, 30]} '
    data = text.encode()
    n = len(data)
    dev = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    scratch, scratch_bytes, counts = _index(dev, n, lib)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [7, 8, 21, 0, -77, -77]  # tokens, brackets, non-numeric bytes, final depth; 4 ints only
    cap = 16
    lists = [torch.full((cap,), -5, dtype=torch.int32, device="cuda") for _ in range(6)]
    tok_pos, tok_brk, brk_pos, brk_key, brk_nonnum, brk_tok = lists
    _lib.check(lib.dad3d_json_parse_lists(dev.data_ptr(), n, scratch.data_ptr(), scratch_bytes, tok_pos.data_ptr(), tok_brk.data_ptr(), cap,
                                          brk_pos.data_ptr(), brk_key.data_ptr(), brk_nonnum.data_ptr(), brk_tok.data_ptr(), cap, 0, None))
    torch.cuda.synchronize()
    outside = text.index('"a"')
    want_tok = [i for i in range(outside, n) if text[i] in "0123456789-" and text[i - 1] in " ["]
    want_brk = [i for i in range(outside, n) if text[i] in "[]"]
    assert tok_pos.cpu().tolist() == want_tok + [-5] * (cap - 7) and brk_pos.cpu().tolist() == want_brk + [-5] * (cap - 8)
    assert tok_brk.cpu().tolist() == [2, 2, 4, 4, 7, 7, 7] + [-5] * 9
    assert brk_key.cpu().tolist() == [1, 2, 2, 2, 2, 1, 1, 1] + [-5] * 8
    assert brk_tok.cpu().tolist() == [0, 0, 2, 2, 4, 4, 4, 7] + [-5] * 8
    assert len(set(brk_nonnum.cpu().tolist()[:6])) == 1 and brk_nonnum.cpu().tolist()[8:] == [-5] * 8
    # a capacity below the counts cuts the lists, it does not overrun them
    small = [torch.full((cap,), -5, dtype=torch.int32, device="cuda") for _ in range(6)]
    _lib.check(lib.dad3d_json_parse_lists(dev.data_ptr(), n, scratch.data_ptr(), scratch_bytes, small[0].data_ptr(), small[1].data_ptr(), 3,
                                          small[2].data_ptr(), small[3].data_ptr(), small[4].data_ptr(), small[5].data_ptr(), 2, 0, None))
    torch.cuda.synchronize()
    assert small[0].cpu().tolist() == want_tok[:3] + [-5] * 13 and small[2].cpu().tolist() == want_brk[:2] + [-5] * 14
    # the two arrays: brackets 0..5 (two rows) and 6..7; a span that is no array gets -1
    arr_open = torch.tensor([0, 6, 1, 0], dtype=torch.int32, device="cuda")
    arr_close = torch.tensor([5, 7, 2, 7], dtype=torch.int32, device="cuda")
    rows = torch.full((8,), -9, dtype=torch.int32, device="cuda")
    _lib.check(lib.dad3d_json_parse_check_arrays(dev.data_ptr(), n, tok_pos.data_ptr(), tok_brk.data_ptr(), 7, brk_pos.data_ptr(), brk_key.data_ptr(),
                                                 brk_tok.data_ptr(), 8, arr_open.data_ptr(), arr_close.data_ptr(), rows.data_ptr(), 4, 0, None))
    torch.cuda.synchronize()
    assert rows.cpu().tolist() == [2, 0, 0, -1] + [-9] * 4
    records = torch.tensor([[want_brk[0], want_brk[5] + 1, 0, 4, 2, 0], [want_brk[6], want_brk[7] + 1, 4, 3, 0, 4]], dtype=torch.int32, device="cuda")
    values = torch.full((12,), -1.5, dtype=torch.float64, device="cuda")
    is_int = torch.full((12,), 9, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dad3d_json_parse_extract(dev.data_ptr(), n, tok_pos.data_ptr(), 7, records.data_ptr(), 2, 7, values.data_ptr(), is_int.data_ptr(), 12,
                                            0, None))
    torch.cuda.synchronize()
    assert values.cpu().tolist() == [1.0, 2.5, 3.0, -400.0, 10.0, 20.0, 30.0] + [-1.5] * 5
    assert is_int.cpu().tolist() == [1, 0, 1, 0, 1, 1, 1] + [9] * 5


def test_c_abi_rejects_bad_arguments_without_device_work():
    lib = _lib.load()
    n = 100
    dev = torch.full((112,), 0x20, dtype=torch.uint8, device="cuda")
    scratch_bytes = lib.dad3d_json_parse_scratch_bytes(n)
    assert scratch_bytes == 112 + 5 * 4 and lib.dad3d_json_parse_scratch_bytes(TILE + 1) == TILE + 16 + 2 * 5 * 4
    assert lib.dad3d_json_parse_scratch_bytes(0) == 0 and lib.dad3d_json_parse_scratch_bytes(2 ** 31) == 0
    scratch = torch.full((scratch_bytes,), 0x55, dtype=torch.uint8, device="cuda")
    counts = torch.full((4,), -77, dtype=torch.int32, device="cuda")
    t, s, c = dev.data_ptr(), scratch.data_ptr(), counts.data_ptr()
    bad = [(None, n, s, scratch_bytes, c), (t, n, None, scratch_bytes, c), (t, n, s, scratch_bytes, None), (t, 0, s, scratch_bytes, c),
           (t, -1, s, scratch_bytes, c), (t, 2 ** 31, s, 2 ** 32, c), (t, n, s, scratch_bytes - 1, c), (t + 1, n, s, scratch_bytes, c),
           (t, n, s + 4, scratch_bytes, c), (t, n, s, scratch_bytes, c + 2)]
    for args in bad:
        lib.dad3d_clear_error()
        assert lib.dad3d_json_parse_index(*args, 0, None) == _lib.E_INVALID, args
        assert lib.dad3d_last_error() != b""
    i32 = torch.full((8,), -5, dtype=torch.int32, device="cuda")
    p = i32.data_ptr()
    assert lib.dad3d_json_parse_lists(t, n, s, scratch_bytes, None, p, 4, p, p, p, p, 4, 0, None) == _lib.E_INVALID
    assert lib.dad3d_json_parse_lists(t, n, s, scratch_bytes, p, p, -1, p, p, p, p, 4, 0, None) == _lib.E_INVALID
    assert lib.dad3d_json_parse_lists(t, n, s, scratch_bytes - 1, p, p, 4, p, p, p, p, 4, 0, None) == _lib.E_INVALID
    assert lib.dad3d_json_parse_check_arrays(t, n, p, p, 4, p, p, p, 4, p, p, None, 1, 0, None) == _lib.E_INVALID
    assert lib.dad3d_json_parse_check_arrays(t, n, p, p, 4, p, p, p, 4, p, p, p, 5, 0, None) == _lib.E_INVALID  # more arrays than brackets
    assert lib.dad3d_json_parse_check_arrays(t, n, p, p, n + 1, p, p, p, 4, p, p, p, 1, 0, None) == _lib.E_INVALID
    f64 = torch.full((4,), -1.5, dtype=torch.float64, device="cuda")
    assert lib.dad3d_json_parse_extract(t, n, p, 4, p, 1, 4, f64.data_ptr(), p, 3, 0, None) == _lib.E_INVALID  # capacity below n_values
    assert lib.dad3d_json_parse_extract(t, n, p, 4, p, 1, 4, None, p, 4, 0, None) == _lib.E_INVALID
    assert lib.dad3d_json_parse_extract(t, n, p, 4, p, 1, 5, f64.data_ptr(), p, 8, 0, None) == _lib.E_INVALID  # more values than tokens
    torch.cuda.synchronize()
    assert (scratch.cpu() == 0x55).all() and counts.cpu().tolist() == [-77] * 4 and i32.cpu().tolist() == [-5] * 8 and f64.cpu().tolist() == [-1.5] * 4


def test_round_trip_with_the_submission_writer(tmp_path):
    rng = np.random.default_rng(77)
    b, n = 3, 37
    points = torch.from_numpy(rng.integers(-20, 300, (b, 68, 2)).astype(np.int32)).cuda()
    vertices = torch.from_numpy((rng.standard_normal((b, n, 3)) * 0.1).astype(np.float32)).cuda()
    lmk68 = torch.from_numpy((rng.standard_normal((b, 68, 3)) * 0.1).astype(np.float32)).cuda()
    rotation = torch.from_numpy(np.linalg.qr(rng.standard_normal((b, 3, 3)))[0].astype(np.float32)).cuda()
    path = str(tmp_path / "submission.json")
    with benchmark_export.SubmissionWriter(path, n_vertices=n, device=0) as w:
        w.add(["a", "b"], points[:2], vertices[:2], lmk68[:2], rotation[:2])
        w.add(["c"], points[2:], vertices[2:], lmk68[2:], rotation[2:])
    doc = json_reader.load(path, device=0, min_count=1)
    assert json.dumps(doc.to_python()) == json.dumps(json.load(open(path))) and len(doc.arrays) == 4 * b
    for i, key in enumerate("abc"):
        entry = doc.root[key]
        assert torch.equal(entry["68_landmarks_2d"].float32(), points[i].float())
        assert torch.equal(entry["N_landmarks_3d"].float32().view(torch.int32), vertices[i].view(torch.int32))
        assert torch.equal(entry["7_landmarks_3d"].float32().view(torch.int32), benchmark_export.seven_landmarks(lmk68[i]).contiguous().view(torch.int32))
        assert torch.equal(entry["rotation_matrix"].float32().view(torch.int32), rotation[i].view(torch.int32))
    doc = json_reader.load(path, device=0)  # the default threshold: the two short fields arrive as lists
    assert len(doc.arrays) == 2 * b and isinstance(doc.root["b"]["rotation_matrix"], list)


def test_evaluator_device_reader_equals_host_reader(tmp_path, monkeypatch):
    golden = er.load_golden()
    gt, sub = er.golden_json(golden)
    sub["1"] = dict(sub["1"], **{"68_landmarks_2d": sub["1"]["68_landmarks_2d"][:-1]})  # one malformed field: 67 points, still a handle
    gt_path, sub_path = str(tmp_path / "gt.json"), str(tmp_path / "submission.json")
    json.dump(gt, open(gt_path, "w"))
    json.dump(sub, open(sub_path, "w"))
    seen = {}
    real = evaluation.evaluate_batch

    def spy(*args, **kwargs):
        seen.setdefault(seen["reader"], []).append([a.clone() for a in args])
        return real(*args, **kwargs)

    monkeypatch.setattr(evaluation, "evaluate_batch", spy)
    results = {}
    for reader in ("host", "device"):
        seen["reader"] = reader
        ev = evaluation.DADEvaluator(gt_path, sub_path, face_indices=golden["face_indices"], batch_size=2, reader=reader)
        results[reader] = (ev(), list(ev.warnings))
    assert results["device"] == results["host"]
    assert [i for i, _ in results["host"][1]] == ["1", "3", "4", "5"]
    assert len(seen["host"]) == len(seen["device"]) > 0
    for host_args, device_args in zip(seen["host"], seen["device"]):  # the tensors handed to evaluate_batch, bit for bit
        for h, d in zip(host_args, device_args):
            assert h.dtype == d.dtype and h.shape == d.shape and torch.equal(h.view(torch.uint8), d.view(torch.uint8))
    # the device reader did lift the fields it gathers from
    doc = json_reader.load(sub_path, device=0)
    assert isinstance(doc.root["0"]["N_landmarks_3d"], json_reader.DeviceArray) and doc.root["1"]["68_landmarks_2d"].shape == (67, 2)
    assert isinstance(json_reader.load(gt_path, device=0).root[0]["vertices"], json_reader.DeviceArray)
    with pytest.raises(ValueError, match="reader"):
        evaluation.DADEvaluator(gt_path, sub_path, face_indices=golden["face_indices"], reader="gpu?")
