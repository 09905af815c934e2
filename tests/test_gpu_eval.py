"""GPU: the benchmark scorer's kernels (csrc/mesh_eval.hip) and `evaluation.DADEvaluator` against the float64 restatement of
tests/eval_restatement.py and the reference's own numbers (tests/golden/eval_golden.npz)."""
import numpy as np
import pytest
import torch

import eval_restatement as er
from dad_3dheads_amd import evaluation, synthetic
from dad_3dheads_amd.benchmark_export import Landmarks68

pytestmark = pytest.mark.gpu

CHAMFER_RTOL = 1e-4  # fp32 kernel distances vs float64 (centred inputs)
NEAR_TIE = 1e-5      # Z5: relative gap between neighbouring sorted distances below which fp32 may order either way


def nn_oracle(q, p, k, self_exclude=False, sim=None):
    q, p = q.astype(np.float64), p.astype(np.float64)
    if sim is not None:
        p = sim[0] * p @ sim[1:10].reshape(3, 3) + sim[10:13]
    d = ((q[:, None] - p[None]) ** 2).sum(-1)
    if self_exclude:
        np.fill_diagonal(d, np.inf)
    o = np.argsort(d, axis=1, kind="stable")[:, :k + 1]  # one more: a tie at rank k shows
    return o, np.take_along_axis(d, o, 1)


def check_knn(idx, dist, o, d, k):
    """Indices equal the oracle's except at near-ties of the oracle's own distances; distances to fp32 rounding. The kernel maps
    the points through the similarity in fp32 (~1e-6 absolute on O(1) coordinates), so both are judged on sqrt(d)."""
    r = np.sqrt(d)
    np.testing.assert_allclose(np.sqrt(dist), r[:, :k], rtol=1e-6, atol=1e-5)  # d, o: k + 1 columns (or all of them)
    tied = np.zeros_like(d, dtype=bool)
    gap = np.diff(r, axis=1) <= 1e-5
    tied[:, 1:] |= gap
    tied[:, :-1] |= gap
    ok = ~tied[:, :k]
    assert np.array_equal(idx[ok], o[:, :k][ok])


@pytest.mark.parametrize("q,n,k", [(300, 1100, 1), (257, 1, 1), (1000, 2049, 5), (64, 3000, 8), (5, 7, 8)])
def test_nearest_matches_oracle(q, n, k):
    rng = np.random.default_rng(q * 7 + n)
    b = 3
    qs = rng.normal(0, 1, (b, q, 3)).astype(np.float32)
    ps = rng.normal(0, 1, (b, n, 3)).astype(np.float32)
    counts = np.array([n, max(1, n // 2), max(1, n - 3)], np.int32)  # ragged
    sim = np.stack([np.concatenate([[rng.uniform(0.5, 2)], np.linalg.qr(rng.normal(size=(3, 3)))[0].ravel(), rng.normal(0, 1, 3)])
                    for _ in range(b)]).astype(np.float32)
    dev = torch.device("cuda", 0)
    mind, idx, dist = evaluation.nearest(torch.from_numpy(qs).to(dev), torch.from_numpy(ps).to(dev), torch.from_numpy(counts).to(dev),
                                         torch.from_numpy(sim).to(dev), k=k, want_knn=True)
    mind, idx, dist = mind.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
    for i in range(b):
        m = counts[i]
        o, d = nn_oracle(qs[i], ps[i, :m], k, sim=sim[i].astype(np.float64))
        kk = min(k, m)
        check_knn(idx[i, :, :kk], dist[i, :, :kk], o, d, kk)
        np.testing.assert_allclose(np.sqrt(mind[i]), np.sqrt(d[:, 0]), rtol=1e-6, atol=1e-5)
        if kk < k:  # fewer points than k
            assert (idx[i, :, kk:] == -1).all() and np.isinf(dist[i, :, kk:]).all()


def test_nearest_self_exclusion_and_ties():
    rng = np.random.default_rng(5)
    pts = rng.normal(0, 1, (1, 700, 3)).astype(np.float32)
    pts[0, 400] = pts[0, 10]  # exact duplicates: the lower index wins a tie
    pts[0, 650] = pts[0, 10]
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(pts).to(dev)
    _, idx, dist = evaluation.nearest(t, t, k=5, self_exclude=True, want_knn=True)
    idx, dist = idx.cpu().numpy()[0], dist.cpu().numpy()[0]
    o, d = nn_oracle(pts[0], pts[0], 5, self_exclude=True)
    check_knn(idx, dist, o, d, 5)
    assert idx[10, 0] == 400 and idx[10, 1] == 650 and dist[10, 0] == 0.0
    assert idx[400, 0] == 10 and idx[400, 1] == 650 and idx[650, 0] == 10 and idx[650, 1] == 400
    assert not (idx == np.arange(700)[:, None]).any()
    _, idx_all, _ = evaluation.nearest(t, t, k=1, want_knn=True)  # without the exclusion every point finds itself (or a lower twin)
    assert idx_all.cpu().numpy()[0, 10, 0] == 10 and idx_all.cpu().numpy()[0, 400, 0] == 10


# ---- exact: lattice inputs (eval_restatement.lattice_points) make every fp32 distance equal float64's, so the kernels are held
# to the bit and to "ties to the lower index" with no near-tie exemption ---------------------------------------------------------
def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype)


def _nearest_np(q, p, counts=None, sim=None, **kw):
    out = evaluation.nearest(_dev(q), _dev(p), None if counts is None else _dev(np.asarray(counts, np.int32)),
                             None if sim is None else _dev(sim), want_knn=True, **kw)
    return tuple(t.cpu().numpy() for t in out)


def _assert_nearest_exact(got, q, p, k, counts=None, sim=None, self_exclude=False):
    mind, idx, dist = got
    for i in range(len(q)):
        m = p.shape[1] if counts is None else min(max(int(counts[i]), 0), p.shape[1])
        o, d = er.nearest_exact(q[i], p[i, :m], k, self_exclude, None if sim is None else sim[i])
        assert np.array_equal(idx[i], o), (i, np.argwhere(idx[i] != o)[:5])
        assert np.array_equal(dist[i], d), i
        assert np.array_equal(mind[i], d[:, 0]), i


# (k, N, Q, with a similarity): every k meets N = 1025 (one point past the LDS tile) and N < k (N == k for k = 1); the other N
# and Q cross sparingly, with and without the similarity
NEAREST_CASES = [(1, 1025, 257, True), (2, 1025, 257, True), (3, 1025, 257, True), (4, 1025, 257, True),
                 (5, 1025, 257, True), (6, 1025, 257, True), (7, 1025, 257, True), (8, 1025, 257, True), (1, 1, 255, False),
                 (2, 1, 1, True), (3, 1, 256, False), (4, 1, 257, True), (5, 1, 255, False), (6, 1, 1, True),
                 (7, 1, 256, False), (8, 7, 257, True), (8, 1, 255, True), (4, 7, 256, True), (1, 7, 1, False),
                 (5, 1023, 256, False), (1, 1024, 256, False), (8, 1024, 257, True), (2, 1023, 1, True),
                 (3, 2049, 255, False), (1, 2049, 257, False), (6, 2049, 1, True), (7, 1024, 255, False)]


@pytest.mark.parametrize("k,n,q,with_sim", NEAREST_CASES)
def test_nearest_exact_on_lattice(k, n, q, with_sim):
    rng = np.random.default_rng(1000 * k + n + q)
    qs, ps = er.lattice_points(rng, q, batch=3), er.lattice_points(rng, n, batch=3)
    sim = None
    if with_sim:  # a reflection first: Procrustes may return one
        sim = np.stack([er.lattice_similarity(rng, det=-1), er.lattice_similarity(rng), er.lattice_similarity(rng)])
    _assert_nearest_exact(_nearest_np(qs, ps, sim=sim, k=k), qs, ps, k, sim=sim)


def test_nearest_ragged_counts_are_clamped_and_rows_past_them_never_read():
    rng = np.random.default_rng(77)
    n, q, k = 1100, 257, 3
    counts = np.array([0, -3, n + 5, 1024, 1025], np.int32)
    qs, ps = er.lattice_points(rng, q, batch=5), er.lattice_points(rng, n, batch=5)
    for i, c in enumerate(counts):
        ps[i, max(int(c), 0):] = np.nan
    sim = np.stack([er.lattice_similarity(rng) for _ in range(5)])
    got = _nearest_np(qs, ps, counts, sim, k=k)
    _assert_nearest_exact(got, qs, ps, k, counts, sim)
    mind, idx, dist = got
    assert (idx[:2] == -1).all() and np.isposinf(dist[:2]).all() and np.isposinf(mind[:2]).all()  # count 0 and below
    assert idx[2].max() > 1025 and idx[3].max() <= 1023 and idx[4].max() <= 1024 and (idx[2:] >= 0).all()
    assert np.isfinite(dist[2:]).all()


@pytest.mark.parametrize("k", [1, 3])
def test_nearest_duplicates_across_the_tile_edge_go_to_the_lower_index(k):
    rng = np.random.default_rng(k)
    ps = er.lattice_points(rng, 2100, batch=1)
    ps[0, 1024] = ps[0, 2048] = ps[0, 1020]
    qs = np.concatenate([ps[:, 1020:1021], ps[:, 1020:1021] + np.float32(0.125), er.lattice_points(rng, 254, batch=1)], 1)
    got = _nearest_np(qs, ps, k=k)
    _assert_nearest_exact(got, qs, ps, k)
    assert got[1][0, 0].tolist() == [1020, 1024, 2048][:k] and (got[2][0, 0] == 0).all()
    assert got[1][0, 1].tolist() == [1020, 1024, 2048][:k]  # the triple again, at a distance of 3/64


@pytest.mark.parametrize("n", [1, 2, 1024, 1025, 2100])
def test_nearest_self_exclusion_in_every_tile(n):
    rng = np.random.default_rng(n)
    ps = er.lattice_points(rng, n, batch=2)
    if n >= 2:
        ps[:, n - 1] = ps[:, 0]  # twins, in different tiles where there are two
    if n > 1500:
        ps[:, 1500] = ps[:, 1030]
    got = _nearest_np(ps, ps, k=5, self_exclude=True)
    _assert_nearest_exact(got, ps, ps, 5, self_exclude=True)
    _, idx, dist = got
    rows = np.arange(n)[None, :, None]
    assert not (idx == rows).any() and not (idx[:, 1024:] == rows[:, 1024:]).any()  # rows past the first tile skip themselves too
    if n == 1:
        assert (idx == -1).all() and np.isposinf(dist).all() and np.isposinf(got[0]).all()
    else:
        assert (idx[:, 0, 0] == n - 1).all() and (idx[:, n - 1, 0] == 0).all() and (dist[:, [0, n - 1], 0] == 0).all()
    if n > 1500:
        assert (idx[:, 1030, 0] == 1500).all() and (idx[:, 1500, 0] == 1030).all() and (dist[:, [1030, 1500], 0] == 0).all()
    # without the flag every point finds itself, or its lower twin
    _, idx_all, _ = _nearest_np(ps, ps, k=1)
    want = np.arange(n)
    want[n - 1] = 0
    if n > 1500:
        want[1500] = 1030
    assert np.array_equal(idx_all[..., 0], np.stack([want, want]))


@pytest.mark.parametrize("with_sim", [False, True])
def test_nearest_reports_only_finite_distances(with_sim):
    """The rule of include/dad3d.h: a point at a NaN or infinite distance is skipped, a non-finite query gets -1 / +inf."""
    rng = np.random.default_rng(31)
    n, q, k = 1100, 300, 4
    qs, ps = er.lattice_points(rng, q, batch=2), er.lattice_points(rng, n, batch=2)
    ps[0, 5, 0] = ps[0, 1030, 2] = np.nan
    ps[0, 1050, 1] = np.inf
    ps[0, 7] = -np.inf
    ps[1, :n - 2] = np.nan  # fewer finite points than k
    qs[:, 3, 1] = np.nan
    qs[:, 7, 0] = np.inf
    sim = np.stack([er.lattice_similarity(rng), er.lattice_similarity(rng)]) if with_sim else None
    got = _nearest_np(qs, ps, sim=sim, k=k)
    _assert_nearest_exact(got, qs, ps, k, sim=sim)
    mind, idx, dist = got
    assert not np.isin(idx[0], [5, 7, 1030, 1050]).any() and (idx[0, [3, 7]] == -1).all() and np.isposinf(dist[0, [3, 7]]).all()
    ok = np.setdiff1d(np.arange(q), [3, 7])
    assert np.array_equal(np.sort(idx[1, ok], 1), np.tile([-1, -1, n - 2, n - 1], (len(ok), 1))) and not np.isnan(dist).any()
    assert np.isposinf(mind[:, [3, 7]]).all() and np.isfinite(mind[:, ok]).all()


Z5_SIZES = [1, 2, 3, 5, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096]


def _z5_np(g, w, anchors):
    counts, order = evaluation.z5_ranks(_dev(g), _dev(w), anchors=anchors, want_order=True)
    return counts.cpu().numpy(), order.cpu().numpy()


def _assert_z5_exact(g, w, anchors):
    counts, order = _z5_np(g, w, anchors)
    for j in range(len(g)):
        with np.errstate(invalid="ignore"):
            o, _ = er.Restatement.anchor_order(g[j], anchors)
        assert np.array_equal(order[j], o), (j, anchors, np.argwhere(order[j] != o)[:5])
        assert np.array_equal(counts[j], er.Restatement.z5_counts(g[j], w[j], o)), (j, anchors)


def _z5_heads(rng, k):
    """B = 3 head sets of falling span: most keys of the second tie, the third also repeats whole vertices."""
    g = np.stack([er.lattice_points(rng, k, span) for span in (16, 2, 0.5)])
    w = np.stack([er.lattice_points(rng, k, span) for span in (16, 2, 0.5)])
    return g, w


@pytest.mark.parametrize("k", Z5_SIZES)
def test_z5_ranks_exact_on_lattice(k):
    rng = np.random.default_rng(k)
    g, w = _z5_heads(rng, k)
    eight = tuple(int(a) % k for a in (k // 2, 0, k - 1, k // 2, 1, k // 3, 1023, 1024))  # one repeated, both ends
    for anchors in [(0,), (k - 1,), eight] + ([evaluation.Z5_ANCHORS] if k > 5 else []):
        _assert_z5_exact(g, w, anchors)


@pytest.mark.parametrize("k", [9, 1025, 2049])
def test_z5_ranks_non_finite_vertices_sort_last(k):
    rng = np.random.default_rng(k)
    g, w = _z5_heads(rng, k)
    nan_at, inf_lo, inf_hi = k - 3, 0, k - 2  # none of them an anchor
    g[0, nan_at, 0] = g[1, nan_at, 2] = np.nan
    g[1:, inf_lo] = g[1:, inf_hi] = np.inf
    w[2, 7, 2] = np.nan
    anchors = evaluation.Z5_ANCHORS
    _assert_z5_exact(g, w, anchors)
    _, order = _z5_np(g, w, anchors)
    assert (order[0, :, -1] == nan_at).all()  # the NaN takes the last rank
    assert (order[1, :, -3:] == [inf_lo, inf_hi, nan_at]).all()  # the +inf pair by index behind every finite one, then the NaN
    assert (order[2, :, -2:] == [inf_lo, inf_hi]).all()


def test_z5_knn_on_lattice_equals_the_restatement(static):
    """`evaluate_batch(z5="knn")` itself, its nearest call and its gather: an identity model-view makes the world mesh the
    lattice mesh, and 2100 head positions in a shuffled order span three LDS tiles."""
    rng = np.random.default_rng(2100)
    b, n_head = 3, 2100
    gt = np.stack([er.lattice_points(rng, 5023, span) for span in (16, 4, 1)])
    pred = np.stack([er.lattice_points(rng, 5023, span) for span in (16, 4, 1)])
    head = rng.permutation(5023)[:n_head]
    eye = np.tile(np.eye(4, dtype=np.float32), (b, 1, 1))
    kw = dict(landmarks=Landmarks68(static["faces"], device=torch.device("cuda", 0)), head_indices=_dev(head),
              face_indices=_dev(np.arange(100)))
    out = evaluation.evaluate_batch(_dev(gt), _dev(eye), _dev(eye), _dev(np.ones((b, 4))), _dev(np.zeros(b, np.float32)),
                                    _dev(np.zeros((b, 68, 2), np.float32)), _dev(pred), _dev(np.full(b, 5023, np.int32)),
                                    _dev(er.lattice_points(rng, 7, batch=b)), _dev(eye[:, :3, :3]), z5="knn", **kw)
    z5 = out["z5"].cpu().numpy()
    for i in range(b):
        want = er.Restatement.z5_knn(-gt[i][head], pred[i][head])
        count = z5[i] * n_head * 5
        assert abs(count - round(count)) < 1e-6 and round(count) == want, (i, count, want)


def test_z5_knn_on_goldens_matches_the_restatement(golden, restatement, static):
    import train_batch_restatement as tbr

    items = [0, 1, 2]
    out = evaluation.evaluate_batch(*_batch_inputs(golden, items, static), **_kw(golden, static), z5="knn")
    z5 = out["z5"].cpu().numpy()
    head = restatement.head
    n = len(head) * 5
    for j, i in enumerate(items):
        # the evaluator's GT frame: the fp32 k-ordered model-view product (test_gpu_projection.py holds the kernel to it)
        g = -tbr.world(golden["gt_vertices"][i], golden["model_view"][i])[head, :3]
        w = golden["pred_vertices"][i][head]
        idx, d = er.nearest_exact(g, g, 6, self_exclude=True)  # one more: a tie at rank 5 shows
        gap = np.diff(d, axis=1) <= NEAR_TIE * np.maximum(d[:, 1:], 1e-30)
        tied = np.zeros_like(d, dtype=bool)
        tied[:, 1:] |= gap
        tied[:, :-1] |= gap
        n_tied = int(tied[:, :5].sum())
        want = int(restatement.knn_agreement(g, w, idx[:, :5]).sum())  # = Restatement.z5_knn(g, w), on the neighbours already found
        count = z5[j] * n
        print(f"item {i}: knn Z5 count {count:.6f}, float64 restatement {want}, near-tied entries {n_tied}")
        assert n_tied <= 5
        assert abs(count - round(count)) < 1e-6 and abs(round(count) - want) <= n_tied
        # the kernel's own neighbours, outside those entries
        _, got, _ = _nearest_np(g[None], g[None], k=5, self_exclude=True)
        print(f"item {i}: kernel neighbours that differ from float64's: {int((got[0] != idx[:, :5]).sum())} (all among the near-tied)")
        assert np.array_equal(got[0][~tied[:, :5]], idx[:, :5][~tied[:, :5]])


@pytest.fixture(scope="module")
def golden():
    return er.load_golden()


@pytest.fixture(scope="module")
def restatement(golden):
    return er.restatement_from_package(golden["face_indices"])


def test_z5_anchor_counts_match_oracle(golden, restatement):
    dev = torch.device("cuda", 0)
    ok = [i for i in range(6) if not np.isnan(golden["per_item"][i, 2])]
    g = np.stack([-restatement.world(golden["gt_vertices"][i], golden["model_view"][i])[restatement.head] for i in ok])
    w = np.stack([golden["pred_vertices"][i][restatement.head] for i in ok])
    counts, order = evaluation.z5_ranks(torch.from_numpy(g).to(dev), torch.from_numpy(w).to(dev), want_order=True)
    counts, order = counts.cpu().numpy(), order.cpu().numpy()
    for j in range(len(ok)):
        o, d = restatement.anchor_order(g[j])
        gap = np.abs(np.diff(d, axis=1)) <= NEAR_TIE * np.maximum(d[:, 1:], 1e-30)
        tied = np.zeros_like(d, dtype=bool)
        tied[:, 1:] |= gap
        tied[:, :-1] |= gap
        assert np.array_equal(order[j][~tied], o[~tied])
        assert np.array_equal(np.sort(order[j], 1), np.tile(np.arange(g.shape[1]), (5, 1)))  # a permutation
        # the counts are exactly the comparisons along the kernel's own order, and the oracle's outside near-ties
        assert np.array_equal(counts[j], restatement.z5_counts(g[j], w[j], order[j]))
        assert np.all(np.abs(counts[j] - restatement.z5_counts(g[j], w[j], o)) <= tied.sum(1))


def _batch_inputs(golden, items, static):
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dt)  # noqa: E731
    return (t(golden["gt_vertices"][items]), t(golden["model_view"][items]), t(golden["projection"][items]),
            t(golden["bbox"][items].astype(np.float64), torch.float64), t(golden["height"][items].astype(np.float32)),
            t(golden["pred_lmk68_2d"][items]), t(golden["pred_vertices"][items]), t(golden["pred_counts"][items], torch.int32),
            t(golden["pred_lmk7"][items]), t(golden["pred_rotation"][items]))


def _kw(golden, static):
    dev = torch.device("cuda", 0)
    return dict(landmarks=Landmarks68(static["faces"], device=dev), head_indices=torch.from_numpy(static["head_indices"]).to(dev),
                face_indices=torch.from_numpy(golden["face_indices"].astype(np.int64)).to(dev))


def test_evaluate_batch_matches_golden_and_oracle(golden, restatement, static):
    items = [0, 1, 2]  # the complete items
    out = evaluation.evaluate_batch(*_batch_inputs(golden, items, static), **_kw(golden, static))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    ref = golden["per_item"][items]
    np.testing.assert_allclose(out["pose_error"], ref[:, 0], rtol=0, atol=1e-6)
    np.testing.assert_allclose(out["nme"], ref[:, 1], rtol=0, atol=1e-5)
    np.testing.assert_allclose(out["chamfer"], ref[:, 3], rtol=CHAMFER_RTOL)
    for j, i in enumerate(items):
        world = restatement.world(golden["gt_vertices"][i], golden["model_view"][i])
        pv = golden["pred_vertices"][i, :golden["pred_counts"][i]]
        assert out["chamfer"][j] == pytest.approx(restatement.chamfer(world, pv, golden["pred_lmk7"][i]), rel=CHAMFER_RTOL)
        assert abs(out["z5"][j] - ref[j, 2]) * 3669 * 5 <= golden["z5_cdist_vs_f64"][i] + 1


def test_batch_equals_items_one_at_a_time(golden, static):
    items = [0, 1, 2, 4]
    kw = _kw(golden, static)
    whole = evaluation.evaluate_batch(*_batch_inputs(golden, items, static), **kw)
    for j, i in enumerate(items):
        one = evaluation.evaluate_batch(*_batch_inputs(golden, [i], static), **kw)
        assert torch.equal(whole["z5"][j:j + 1], one["z5"]), i
        assert one["chamfer"].item() == pytest.approx(whole["chamfer"][j].item(), rel=1e-12), i
    # the kernels themselves: one launch over the batch writes the same bits as one launch per item
    rng = np.random.default_rng(9)
    q = torch.from_numpy(rng.normal(0, 1, (4, 500, 3)).astype(np.float32)).cuda()
    p = torch.from_numpy(rng.normal(0, 1, (4, 1500, 3)).astype(np.float32)).cuda()
    cnt = torch.tensor([1500, 1200, 7, 1499], dtype=torch.int32, device="cuda")
    sim = torch.from_numpy(rng.normal(0, 1, (4, 13)).astype(np.float32)).cuda()
    full = evaluation.nearest(q, p, cnt, sim, k=3, want_knn=True)
    zc, zo = evaluation.z5_ranks(q, p[:, :500].contiguous(), want_order=True)
    for i in range(4):
        one = evaluation.nearest(q[i:i + 1], p[i:i + 1], cnt[i:i + 1], sim[i:i + 1], k=3, want_knn=True)
        assert all(torch.equal(a[i:i + 1], b) for a, b in zip(full, one)), i
        c1, o1 = evaluation.z5_ranks(q[i:i + 1], p[i:i + 1, :500].contiguous(), want_order=True)
        assert torch.equal(zc[i:i + 1], c1) and torch.equal(zo[i:i + 1], o1), i
    kn = evaluation.evaluate_batch(*_batch_inputs(golden, items, static), **kw, z5="knn")
    assert torch.equal(kn["chamfer"], whole["chamfer"]) and not torch.equal(kn["z5"], whole["z5"])


def test_sanity_identities(golden, static):
    """prediction = -(GT world): Z5 = 1 exactly, Chamfer ~ 0; the GT landmarks as prediction: NME = 0; R_pred = R_gt: pose 0."""
    items = [0, 1]
    kw = _kw(golden, static)
    args = list(_batch_inputs(golden, items, static))
    gt_v, mv, pm, height = args[0], args[1], args[2], args[4]
    world = evaluation.project_batch(gt_v, mv, pm, height, want_world=True)["world"][..., :3]
    pred_v = (-world).contiguous()
    args[6] = pred_v
    args[7] = torch.full((2,), 5023, dtype=torch.int32, device="cuda:0")
    args[8] = kw["landmarks"](pred_v)[:, list(evaluation.SEVEN_OF_68)].contiguous()
    args[5] = evaluation.project_batch(kw["landmarks"](gt_v).contiguous(), mv, pm, height)["xy"]
    args[9] = (mv.double()[:, :3, :3] * torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64, device="cuda:0")[None, :, None]).float()
    out = evaluation.evaluate_batch(*args, **kw)
    assert torch.all(out["z5"] == 1.0)
    assert torch.all(out["nme"] == 0.0)
    assert torch.all(out["pose_error"] < 1e-6)
    assert torch.all(out["chamfer"] < 1e-6), out["chamfer"]
    kn = evaluation.evaluate_batch(*args, **kw, z5="knn")
    assert torch.all(kn["z5"] == 1.0)


def test_dad_evaluator_reproduces_the_reference(golden, tmp_path):
    import json

    gt_path, sub_path = er.write_golden_json(golden, str(tmp_path))
    ev = evaluation.DADEvaluator(gt_path, sub_path, face_indices=golden["face_indices"], batch_size=2)
    overall, attribute = ev()
    ref_o, ref_a = json.loads(str(golden["overall"])), json.loads(str(golden["attribute"]))
    assert list(overall) == list(ref_o) and list(attribute) == list(ref_a)
    tol = {"pose_error": dict(rel=0, abs=1e-6), "nme_reprojection": dict(rel=0, abs=1e-5), "chamfer": dict(rel=CHAMFER_RTOL)}
    z5_slack = golden["z5_cdist_vs_f64"].sum() / (3669 * 5)  # the script's cdist noise, whole set
    for name, v in overall.items():
        if name == "z5_accuracy":
            assert abs(v - ref_o[name]) <= z5_slack
        else:
            assert v == pytest.approx(ref_o[name], **tol[name])
    for name, per in attribute.items():
        assert {a: set(vals) for a, vals in per.items()} == {a: set(vals) for a, vals in ref_a[name].items()}
        for a, vals in per.items():
            for val, v in vals.items():
                if name == "z5_accuracy":
                    assert abs(v - ref_a[name][a][val]) <= z5_slack
                else:
                    assert v == pytest.approx(ref_a[name][a][val], **tol[name])
    assert [i for i, _ in ev.warnings] == ["3", "4", "5"]
