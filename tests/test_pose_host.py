"""CPU: the head-pose and Procrustes routines of csrc/pose_math.hpp through their host entries (`dad3d_head_pose_host`,
`dad3d_procrustes_host`: the code the kernels of csrc/head_pose.hip run), held to the numpy statement in dad_3dheads_amd/pose.py,
and that statement held to scipy and to `evaluation.procrustes`."""
import numpy as np
import pytest
import torch

import pose_restatement as pr
from dad_3dheads_amd import _lib, overlay, pose

NF, DG, GB, IX = _lib.POSE_FLAG_NONFINITE, _lib.POSE_FLAG_DEGENERATE, _lib.POSE_FLAG_GIMBAL, _lib.POSE_FLAG_INDEX
N_ROWS = 6000


@pytest.fixture(scope="module")
def rows():
    return pr.rot6_rows(N_ROWS)


@pytest.fixture(scope="module")
def statement(rows):
    rpy, flags = pose.rpy_rows(rows)
    rpy.setflags(write=False)
    return rpy, flags


def test_statement_of_scipys_route_matches_scipy(rows):
    """At least 5000 seeded rows whose second Euler angle is at least 1 degree from +-90: within 1e-9 degrees of scipy."""
    matrices = np.transpose(pose.rotation_rows(rows), (0, 2, 1))
    ref = pr.scipy_euler(matrices)
    far = np.abs(np.abs(ref[:, 1]) - 90.0) >= 1.0
    assert far.sum() >= 5000
    got, flags = pose.euler_rows(matrices)
    assert np.all(flags[far] == 0)
    diff = np.abs(got - ref)[far].max()
    print(f"statement vs scipy over {far.sum()} rows: max {diff:.3g} degrees")
    assert diff <= pr.RPY_TOL_DEG


def test_statement_without_the_polar_factor_is_not_scipy(rows):
    """Why the route is followed step for step: the same formulas on the float32 matrix as it is are off by far more than the bound."""
    matrices = np.transpose(pose.rotation_rows(rows[:2000]), (0, 2, 1)).astype(np.float64)
    ref = pr.scipy_euler(matrices)
    raw = np.array([[a * 180.0 / np.pi for a in pose.euler_xyz_from_quat(pose.quat_from_matrix(m))[0]] for m in matrices])
    far = np.abs(np.abs(ref[:, 1]) - 90.0) >= 1.0
    assert np.abs(raw - ref)[far].max() > 1e-6


@pytest.mark.parametrize("angle,want", [(180.0, 180.0), (-180.0, -180.0), (360.0, 0.0), (-360.0, 0.0), (-350.0, 10.0), (540.0, -180.0),
                                        (0.0, 0.0), (-0.0, -0.0), (190.0, -170.0), (-190.0, 170.0), (-540.0, 180.0), (179.5, 179.5)])
def test_limit_angle_hand_cases(angle, want):
    """flame.py:239-251: int() truncates toward zero, // floors, exactly +-180 stays. The host entry's limit_angle is reached
    through its rpy below; here the statement and the overlay's own copy."""
    for fn in (pose.limit_angle, overlay.limit_angle):
        got = fn(angle)
        assert got == want and np.signbit(got) == np.signbit(want), (fn.__module__, angle, got)


def test_host_entry_matches_the_statement(rows, statement):
    rpy, flags = statement
    got = pose.head_pose_host(rows, size=(480, 640))
    assert got.rotation.dtype == np.float32 and got.rpy.dtype == np.float64 and got.points.dtype == np.float32
    assert np.array_equal(got.rotation.view(np.uint32), pose.rotation_rows(rows).view(np.uint32))  # bit for bit
    assert np.array_equal(got.flags, flags) and np.all(flags == 0)
    diff = np.abs(got.rpy - rpy).max()
    print(f"host entry vs statement: rpy max {diff:.3g} degrees")
    assert diff <= pr.RPY_TOL_DEG
    ref = pr.reference_rpy(rows)
    far = np.abs(np.abs(ref[:, 2]) - 90.0) >= 1.0  # yaw is the second Euler angle
    assert far.sum() >= 5000 and np.abs(got.rpy - ref)[far].max() <= pr.RPY_TOL_DEG  # scipy itself
    pr.assert_points(got.points, rpy, (480, 640), "uniform size")


def test_host_entry_points_per_frame_and_strided_params(rows, statement):
    """A frame table with three sizes and an image_index with -1 and one index beyond the table; the rows inside a [n,413] array."""
    rpy, _ = statement
    n = 700
    sizes = [(480, 640), (200, 333), (1081, 1919)]
    index = np.random.default_rng(3).integers(0, 3, n).astype(np.int32)
    index[5], index[77] = -1, 3
    params = np.random.default_rng(4).standard_normal((n, pose.N_PARAMS)).astype(np.float32)
    params[:, pose.ROTATION_OFFSET:pose.ROTATION_OFFSET + 6] = rows[:n]
    got = pose.head_pose_host(params, frame_sizes=sizes, image_index=index)
    bare = pose.head_pose_host(rows[:n], size=(480, 640))
    assert np.array_equal(got.rotation, bare.rotation) and np.array_equal(got.rpy, bare.rpy)
    lost = (index < 0) | (index >= 3)
    assert np.array_equal(got.flags, np.where(lost, IX, 0))
    assert np.all(got.points[lost] == 0)
    live = np.flatnonzero(~lost)
    pr.assert_points(got.points[live], rpy[live], [sizes[i] for i in index[live]], "frame table")
    # the overlay's own host points: the same table where no coordinate sits at an edge
    raw = pr.raw_points(rpy[live[:300]], [sizes[i] for i in index[live[:300]]])
    mine = np.stack([overlay.pose_points(overlay.RPY(*rpy[k]), *sizes[index[k]]) for k in live[:300]])
    ok = ~pr.near_edge(raw)
    assert np.array_equal(mine[ok].astype(np.float32), got.points[live[:300]][ok])


# measured on this CPU over the 4096 conditioned rows, as one batch and row by row (the larger of the two): 3.65e-07
ROTATION_VS_FRAMEWORK = 3.65e-07


def test_rotation_against_the_frameworks_six_dof():
    """`autograd.six_dof_to_matrix` (F.normalize + linalg.cross) is not the device's float32 rule to the bit; on rows with |v1| >=
    0.1 and v1, v2 at least 0.1 rad from parallel it stays within four times the deviation measured here (the factor leaves room
    for another batch size's vectorisation)."""
    from dad_3dheads_amd.autograd import six_dof_to_matrix

    rows = pr.conditioned_rows(4096)
    got = pose.head_pose_host(rows, want=("rotation",)).rotation
    t = torch.from_numpy(rows)
    batch = six_dof_to_matrix(t).numpy()
    single = np.concatenate([six_dof_to_matrix(t[i:i + 1]).numpy() for i in range(0, 4096, 16)])
    dev = max(np.abs(got - batch).max(), np.abs(got[::16] - single).max())
    print(f"rotation vs six_dof_to_matrix: max {dev:.3g} (batch {np.abs(got - batch).max():.3g}, single {np.abs(got[::16] - single).max():.3g})")
    assert dev <= 4 * ROTATION_VS_FRAMEWORK


@pytest.mark.parametrize("n_points", pr.PROCRUSTES_COUNTS)
def test_procrustes_host_entry_matches_evaluation_procrustes(n_points):
    x, y = pr.procrustes_inputs(n_points)
    pr.assert_procrustes(pose.procrustes_host(x, y), x, y, what=f"n = {n_points}")


def test_procrustes_item_does_not_depend_on_the_batch():
    x, y = pr.procrustes_inputs(65)
    whole = pose.procrustes_host(x, y)
    for i in (0, 5, 11):
        one = pose.procrustes_host(x[i:i + 1], y[i:i + 1])
        assert all(np.array_equal(a[i:i + 1], b) for a, b in zip(whole, one)), i


def test_procrustes_planar_collinear_and_degenerate_sets():
    rng = np.random.default_rng(8)
    flat = rng.standard_normal((6, 9, 3))
    flat[..., 2] = 0.25                                   # planar
    line = np.linspace(-1, 1, 9)[None, :, None] * rng.standard_normal((6, 1, 3)) + 0.5  # collinear
    for name, x in (("planar", flat), ("collinear", line)):
        y = 0.7 * x[:, :, [1, 2, 0]] + 2.0
        b, t, c, flags = pose.procrustes_host(x, y)
        assert np.all(flags == 0), name
        assert np.isfinite(b).all() and np.isfinite(t).all() and np.isfinite(c).all(), name
        assert np.abs(np.einsum("bji,bjk->bik", t, t) - np.eye(3)).max() <= 1e-12, name
        assert np.abs(pr.aligned(y, b, t, c) - x).max() <= 1e-9, name  # y is an exact similarity copy: the fit reproduces x
    one = rng.standard_normal((3, 1, 3))
    same = np.tile(rng.standard_normal((3, 1, 3)), (1, 7, 1))
    other = rng.standard_normal((3, 7, 3))
    for x, y in ((one, one + 1.0), (same, other), (other, same)):
        b, t, c, flags = pose.procrustes_host(x, y)
        assert np.all(flags == DG) and np.isnan(b).all() and np.isnan(t).all() and np.isnan(c).all()
    bad = other.copy()
    bad[1, 3, 0] = np.inf
    assert list(pose.procrustes_host(bad, other)[3]) == [0, DG, 0]


def test_flags_of_bad_rows():
    good = pr.rot6_rows(8).copy()
    rows = np.tile(good[:1], (7, 1))
    rows[1, 2] = np.nan
    rows[2, 4] = np.inf
    rows[3, :3] = 0.0                       # a zero v1
    rows[4] = [1.5, 1.5, 1.5, -3.0, -3.0, -3.0]  # v2 parallel to v1, exactly: the cross product is 0
    rows[5, 3:] = 0.0                       # a zero v2
    got = pose.head_pose_host(rows, size=(300, 400))
    assert list(got.flags) == [0, NF, NF, DG, DG, DG, 0]
    bad = got.flags != 0
    assert np.isnan(got.rpy[bad]).all() and np.isfinite(got.rpy[~bad]).all()
    assert np.all(got.points[bad] == np.array([200.0, 150.0], np.float32))  # all ten at the frame's centre
    _, flags = pose.rpy_rows(rows)
    assert np.array_equal(flags, got.flags)
    # scipy raises on what DEGENERATE marks
    from scipy.spatial.transform import Rotation
    for k in (3, 4, 5):
        with pytest.raises(ValueError):
            Rotation.from_matrix(got.rotation[k].T.astype(np.float64))


def test_exact_lock_matrices_take_the_gimbal_branch():
    """GIMBAL is set, and the returned angles rebuild the polar factor of the input within 1e-6 (they need not be scipy's one by
    one: at the lock only the sum or the difference of the first and third angle is defined)."""
    from scipy.spatial.transform import Rotation

    rows = pr.lock_rows()
    got = pose.head_pose_host(rows, size=(300, 400))
    assert np.all(got.flags == GB), got.flags
    assert np.all(np.abs(np.abs(got.rpy[:, 2]) - 90.0) <= 1e-5)  # yaw, the second Euler angle
    for k, (roll, pitch, yaw) in enumerate(got.rpy):
        m = got.rotation[k].T.astype(np.float64)
        u, _, vt = np.linalg.svd(m)
        rebuilt = Rotation.from_euler("xyz", [pitch + 180.0, yaw, roll], degrees=True).as_matrix()
        assert np.abs(rebuilt - u @ vt).max() <= 1e-6, (k, got.rpy[k])
    _, flags = pose.rpy_rows(rows)
    assert np.array_equal(flags, got.flags)


def test_argument_checks_come_before_any_work():
    lib = _lib.load()
    rows = pr.rot6_rows(4).copy()
    out = np.zeros((4, 10, 2), np.float32)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert lib.dad3d_head_pose_host(None, 4, 6, 0, None, 0, None, 10, 10, None, None, None, None) == _lib.E_INVALID
    assert lib.dad3d_head_pose_host(p(rows), 4, 6, 0, None, 0, None, 0, 10, None, None, p(out), None) == _lib.E_INVALID  # points, no size
    assert lib.dad3d_head_pose_host(p(rows), -1, 6, 0, None, 0, None, 10, 10, None, None, None, None) == _lib.E_INVALID
    assert lib.dad3d_head_pose_host(p(rows), 4, 6, 0, p(np.zeros(4, np.int64)), 1, None, 0, 0, None, None, None, None) == _lib.E_INVALID
    assert lib.dad3d_head_pose_host(p(rows), 0, 6, 0, None, 0, None, 0, 0, None, None, None, None) == _lib.OK
    assert lib.dad3d_head_pose(None, 4, 6, 0, None, 0, None, 10, 10, None, None, None, None, 0, None) == _lib.E_INVALID
    x = np.zeros((2, 3, 3))
    assert lib.dad3d_procrustes_host(p(x), p(x), 2, 0, p(x), p(x), p(x), p(x)) == _lib.E_INVALID
    assert lib.dad3d_procrustes_host(p(x), None, 2, 3, p(x), p(x), p(x), p(x)) == _lib.E_INVALID
    assert lib.dad3d_procrustes(None, None, 2, 3, None, None, None, None, 0, None) == _lib.E_INVALID
    assert lib.dad3d_procrustes_host(None, None, 0, 3, None, None, None, None) == _lib.OK
