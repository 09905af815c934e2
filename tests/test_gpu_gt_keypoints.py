"""GPU: `dad3d_gt_keypoints` (csrc/train_batch.hip) called directly, held to the bit to the NumPy restatement of its fixed fp32 / fp64
order (`train_batch_restatement.chain`) on the cases of tests/gt_keypoints_cases.py -- which tests/test_train_batch_host.py certifies
on the CPU to tell ten restated mistakes from the chain. Every output lies between guard words, and the vertices lie inside a larger
allocation filled with a finite number, so that a stray read shows as a finite point where the header promises NaN."""
import numpy as np
import pytest
import torch

import gt_keypoints_cases as gk
from dad_3dheads_amd import _lib
from dad_3dheads_amd.dataset import RESIZE_MODES
from guarded import Guarded

pytestmark = pytest.mark.gpu
AROUND = 12345.0  # what lies before and behind the vertices
PAD = 64


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


class Launch:
    """One case on the device: inputs uploaded, outputs between guards. `call(**overrides)` hands the entry its 18 arguments."""

    def __init__(self, case, sub=None, items=None):
        sub = gk.subset_of(case) if sub is None else sub
        pick = slice(None) if items is None else items
        verts = case["vertices"][pick]
        self.b, self.nver = verts.shape[:2]
        self.k = len(sub.get("index", sub.get("corners", ())))
        self.around = torch.full((2 * PAD + verts.size,), AROUND, dtype=torch.float32, device="cuda")
        self.around[PAD:PAD + verts.size] = _dev(verts, np.float32).reshape(-1)
        self.keep = [_dev(case["model_view"][pick], np.float32), _dev(case["projection"][pick], np.float32), _dev(case["frames"][pick], np.int32)]
        self.keep += [_dev(sub[key], np.int32 if key != "weights" else np.float32) if key in sub else None for key in ("index", "corners", "weights")]
        b, n, k = self.b, self.nver, self.k
        self.out = {"full": Guarded(b * n * 2, torch.float32), "subset_px": Guarded(b * k * 2, torch.float32),
                    "subset_norm": Guarded(b * k * 2, torch.float32), "presence": Guarded(b * k, torch.uint8)}
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self.args = {"vertices": self.around.data_ptr() + 4 * PAD, "model_view": ptr(self.keep[0]), "projection": ptr(self.keep[1]),
                     "frames": ptr(self.keep[2]), "batch": b, "nver": n, "index": ptr(self.keep[3]), "corners": ptr(self.keep[4]),
                     "weights": ptr(self.keep[5]), "n_subset": k, "out_size": case["size"], "resize_mode": RESIZE_MODES[case["mode"]],
                     "full": self.out["full"].ptr() if n else None, "subset_px": self.out["subset_px"].ptr() if k else None,
                     "subset_norm": self.out["subset_norm"].ptr() if k else None, "presence": self.out["presence"].ptr() if k else None}

    def call(self, **overrides):
        a = dict(self.args, **overrides)
        status = _lib.load().dad3d_gt_keypoints(*(a[key] for key in self.args), 0, None)
        torch.cuda.synchronize()
        return status

    def results(self):
        """(full, subset_px, subset_norm, presence) as the restatement shapes them; the guards are checked on the way."""
        b, n, k = self.b, self.nver, self.k
        full, px, norm, pres = (self.out[key].host() for key in ("full", "subset_px", "subset_norm", "presence"))
        return full.reshape(b, n, 2), px.reshape(b, k, 2), norm.reshape(b, k, 2), pres.reshape(b, k)

    def untouched(self):
        return all((g.host() == g.sentinel).all() for g in self.out.values())


def run(case, **kw):
    launch = Launch(case, **kw)
    assert launch.call() == _lib.OK, _lib.load().dad3d_last_error()
    full, px, norm, pres = launch.results()
    assert set(np.unique(pres).tolist()) <= {0, 1}
    return full, px, norm, pres.astype(bool)


def assert_equal_to_chain(case, got, want=None):
    want = gk.expected(case) if want is None else want
    for what, g, w in zip(("full", "subset_px", "subset_norm", "presence"), got, want):
        assert g.shape == w.shape, (case["name"], what)
        if not gk.same_bits(g, w):
            at = np.argwhere((g != w) & ~(np.isnan(g) & np.isnan(w)) if g.dtype != bool else g != w)
            raise AssertionError(f"{case['name']}: {what} differs in {len(at)} words, first at {at[:4].tolist()}: "
                                 f"{[g[tuple(i)] for i in at[:4]]} for {[w[tuple(i)] for i in at[:4]]}")


# ---- equality with the chain -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, mode, size", [(k, m, s) for k in gk.SUBSETS for m in gk.MODES for s in gk.SIZES])
def test_posed_cases_equal_the_chain_bit_for_bit(kind, mode, size):
    """Seeded cameras, three crops (a negative corner, a 1-px-wide crop, w > h and h > w) at eight (nver, K) shapes: the block where
    subset lanes and vertex lanes meet, K = 0 and nver = 0 (their outputs NULL), partial last blocks, the builder's own shapes."""
    cases = [c for c in gk.posed_cases() if c["name"].startswith(f"posed-{kind}-{mode}-{size}-")]
    assert len(cases) == len(gk.SHAPES)
    for case in cases:
        assert_equal_to_chain(case, run(case))


def test_other_cases_equal_the_chain_bit_for_bit():
    """Exact edges, ids out of range, the camera plane and infinite matrices, homogeneous rows with w = 2."""
    for case in gk.edge_cases() + gk.bad_id_cases() + gk.special_cases():
        assert_equal_to_chain(case, run(case))


def test_exact_edges_against_the_table_written_by_hand():
    """0, -0.0, w, h and one ulp either side of each in crop pixels, index and 68-landmark mode: presence is strict and is taken
    before the resize (a point one pixel outside the padded short side lies inside the resized image)."""
    for case in gk.edge_cases():
        _, px, _, pres = run(case)
        assert np.array_equal(pres, case["presence"]), (case["name"], np.flatnonzero(pres[0] != case["presence"][0]))
        if case["mode"] == "longest_max_size":
            outside = np.flatnonzero(np.abs(case["points"][:, 0] - gk.EDGE_W / 2) == gk.EDGE_W / 2 + 1)
            assert len(outside) == 2 and ((0 < px[0, outside, 0]) & (px[0, outside, 0] < case["size"])).all() and not pres[0, outside].any()


# ---- ids out of range ------------------------------------------------------------------------------------------------------
def test_ids_out_of_range_give_nan_rows_and_read_nothing():
    """-1, nver, INT32_MAX and INT32_MIN, each between good neighbours; in 68-landmark mode one bad corner of three, in each place,
    poisons its landmark. What lies around the vertices is finite, and so is the next item's vertex 0: a read would show."""
    for case in gk.bad_id_cases():
        full, px, norm, pres = run(case)
        bad = case["bad"]
        assert np.isnan(px[:, bad]).all() and np.isnan(norm[:, bad]).all() and not pres[:, bad].any(), case["name"]
        clean = run(case, sub=case["clean"])
        assert np.isfinite(clean[1]).all() and np.array_equal(full.view(np.uint32), clean[0].view(np.uint32))
        for got, want in zip((px, norm, pres), clean[1:]):  # the neighbours: the bits of a run without the bad ids
            assert gk.same_bits(np.ascontiguousarray(got[:, ~bad]), np.ascontiguousarray(want[:, ~bad])), case["name"]
    for case in gk.posed_cases():
        if case["vertices"].shape[1] == 0 and case["size"] == 256:  # no vertex at all: every id is out of range
            full, px, norm, pres = run(case)
            assert np.isnan(px).all() and np.isnan(norm).all() and not pres.any(), case["name"]


# ---- the item axis ---------------------------------------------------------------------------------------------------------
def test_item_of_a_batch_of_70_equals_the_item_launched_alone():
    case = gk.batch_case()
    whole = run(case)
    assert_equal_to_chain(case, whole)
    for i in (0, 1, 35, 69):
        alone = run(case, items=slice(i, i + 1))
        for got, want in zip(alone, whole):
            assert gk.same_bits(got[0], want[i]), i


# ---- the argument contract -------------------------------------------------------------------------------------------------
def test_refused_calls_write_no_word():
    index_case = gk.by_name("posed-index-longest_max_size-256-188-68")
    bary_case = gk.by_name("posed-barycentric-longest_max_size-256-188-68")
    for case in (index_case, bary_case):
        launch = Launch(case)
        spare = launch.keep[2].data_ptr()  # any valid device pointer
        refused = [{"resize_mode": 2}, {"resize_mode": -1}, {"batch": 65536}, {"out_size": 0}, {"out_size": -256}, {"batch": -1}, {"nver": -1},
                   {"n_subset": -1}, {"vertices": None}, {"model_view": None}, {"projection": None}, {"frames": None}, {"full": None},
                   {"subset_px": None}, {"subset_norm": None}, {"presence": None}]
        if case is index_case:
            refused += [{"corners": spare}, {"corners": spare, "weights": spare}, {"weights": spare}, {"index": None}]
        else:
            refused += [{"index": spare}, {"weights": None}, {"corners": None}, {"corners": None, "weights": None}]
        for kw in refused:
            assert launch.call(**kw) == _lib.E_INVALID, (case["name"], kw)
        assert launch.call(batch=0) == _lib.OK
        assert launch.untouched(), "a refused call wrote"
        assert launch.call() == _lib.OK  # and the same buffers serve a good call
        assert_equal_to_chain(case, tuple(a.astype(bool) if a.dtype == np.uint8 else a for a in launch.results()))
