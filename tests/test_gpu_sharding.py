"""GPU box: the multi-GPU path on the hardware there is -- one rank, but the REAL backend. A world-1 "nccl" (= RCCL)
process group runs init_process_group(device_id=...), all_gather_into_tensor and barrier on an MI355X; the sharded
decoders are built under it and compared with the CPU oracle; bench.py is launched the way the driver launches it."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from render_checks import assert_render_bytes_explained

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def nccl_world1():
    import torch.distributed as dist

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def head_mesh(static, flame_model):
    from dad_3dheads_amd import landmarks
    from dad_3dheads_amd.head_mesh import HeadMesh

    return HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)


def test_direct_rccl_all_gather_on_the_launch_stream(nccl_world1, head_mesh):
    """rccl.RcclAllGather: communicator from ncclCommInitRank (unique id through the torch group), ncclAllGather queued on a
    side stream behind a decode launched there -- the gathered landmarks are what that launch wrote, and the sharded decoder
    gives the same tensor through either gather."""
    from dad_3dheads_amd import sharding, synthetic
    from dad_3dheads_amd.rccl import RcclAllGather

    rg = RcclAllGather()
    assert rg.world == 1 and rg.rank == 0
    side = torch.cuda.Stream()
    params = torch.from_numpy(synthetic.synthetic_params(64, seed=77)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        px = head_mesh.decode(params, verts3d=False, proj=False, landmarks=False, landmarks_px=True, mutate=False)["lmk_px"]
        out = torch.empty_like(px)
        rg.all_gather(out, px, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(out, px) and int(px.abs().max()) > 0
    for dtype in (torch.uint8, torch.float32):  # any dtype: moved as bytes
        x = (torch.arange(3 * 5 * 7, device="cuda") % 251).to(dtype).reshape(3, 5, 7)
        assert torch.equal(rg.all_gather(torch.empty_like(x), x), x)
    with pytest.raises(ValueError):
        rg.all_gather(torch.empty(5, device="cuda"), torch.empty(6, device="cuda"))
    # gather-to-root (configs[4]'s default collective): in a world of one the root's own rows, a device copy on the given stream
    img = (torch.arange(4 * 16 * 16 * 3, device="cuda") % 251).to(torch.uint8).reshape(4, 16, 16, 3)
    with torch.cuda.stream(side):
        dst = torch.zeros_like(img)
        assert rg.gather_to_root(dst, img, root=0, stream=side.cuda_stream) is dst
    side.synchronize()
    assert torch.equal(dst, img)
    with pytest.raises(ValueError):
        rg.gather_to_root(None, img, root=0)
    with pytest.raises(ValueError):
        rg.gather_to_root(dst, img, root=1)
    a = sharding.ShardedLandmarkDecoder(head_mesh)(params)
    b = sharding.ShardedLandmarkDecoder(head_mesh, direct_rccl=True)(params)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    rg.destroy()


def test_sharded_landmark_decoder_under_rccl_matches_oracle(nccl_world1, head_mesh, flame_consts, static):
    """BASELINE config 4's per-rank code path: shard -> fused decode -> ONE all_gather_into_tensor on RCCL."""
    from dad_3dheads_amd import sharding, synthetic
    from oracle import flame_ref

    dec = sharding.ShardedLandmarkDecoder(head_mesh)
    for n in (64, 37):
        params = torch.from_numpy(synthetic.synthetic_params(n, seed=300 + n))
        dev_params = params.cuda()
        before = dev_params.clone()
        got = dec(dev_params)
        torch.cuda.synchronize()
        assert got.shape == (n, 445, 2) and got.dtype == torch.int32 and got.is_cuda
        assert torch.equal(dev_params, before)  # a landmark decode does not zero translation z in the caller's rows
        proj = flame_ref.reprojected_vertices(flame_consts, params.clone(), to_2d=True)
        want = flame_ref.gather_landmarks_int(proj, static["lmk_445"]).astype(np.int32)
        lm = proj.numpy()[:, static["lmk_445"], :]
        diff = got.cpu().numpy() != want
        # integer pixels: equal, except where the float coordinate sits within 1e-3 px of an integer (fp32 evaluation order)
        assert np.all(np.abs(lm - np.round(lm))[diff] < 1e-3) and diff.mean() < 1e-3
    # a CPU tensor (every rank holds the global batch on the host) takes the same path
    assert torch.equal(dec(params), got)


def test_sharded_renderer_under_rccl_matches_oracle(nccl_world1, head_mesh, flame_consts, static, sim3dr_oracle):
    """BASELINE config 5's per-rank code path: decode -> normals + Phong + raster -> all-gather of uint8 images."""
    from dad_3dheads_amd import sharding, synthetic
    from dad_3dheads_amd.Sim3DR import Mesh
    from oracle import flame_ref, sim3dr_ref

    faces = static["faces"]
    mesh = Mesh(faces, 5023, device=0)
    renderer = sharding.ShardedRenderer(head_mesh, mesh)
    n = 5
    params = torch.from_numpy(synthetic.synthetic_params(n, seed=512))
    imgs = renderer(params.cuda())
    torch.cuda.synchronize()
    assert imgs.shape == (n, 256, 256, 3) and imgs.dtype == torch.uint8
    verts = flame_ref.reprojected_vertices(flame_consts, params.clone(), to_2d=False).numpy().copy()
    verts[..., 2] *= -1.0  # demo_utils.get_vertices_for_render
    for i in (0, n - 1):
        # the oracle renders the GPU's own decoded vertices (decode parity has its own tests; this one is about the chain)
        v_gpu = np.ascontiguousarray(renderer._dec["proj"][i].cpu().numpy())
        assert np.abs(v_gpu - verts[i]).max() < 1e-3
        ref, ref_light = sim3dr_ref.render_pipeline_ref(sim3dr_oracle, v_gpu.copy(), faces, np.zeros((256, 256, 3), np.uint8))
        assert_render_bytes_explained(imgs[i].cpu().numpy(), ref, sim3dr_oracle, v_gpu, faces, ref_light)
    again = renderer(params.cuda())  # buffers are reused: same bytes
    assert torch.equal(again, imgs)
    for direct in (False, True):  # the images end up on rank 0 only: torch.distributed.gather / grouped ncclSend + ncclRecv
        at_root = sharding.ShardedRenderer(head_mesh, mesh, root=0, direct_rccl=direct)(params.cuda())
        torch.cuda.synchronize()
        assert torch.equal(at_root, imgs)


def test_kernel_attributes_follow_the_device_not_the_process(static, flame_model):
    """MaxDynamicSharedMemorySize is raised per device. With one GPU this exercises the bookkeeping:
    handles created and launched with different 'current device' states around them all run the 150 KB-LDS kernels."""
    import ctypes as C

    from dad_3dheads_amd import _lib, landmarks, synthetic
    from dad_3dheads_amd.head_mesh import HeadMesh
    from dad_3dheads_amd.Sim3DR import Mesh

    lib = _lib.load()
    outs = []
    for _ in range(2):
        torch.cuda.set_device(0)
        hm = HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)
        mesh = Mesh(static["faces"], 5023, device=0)
        p = torch.from_numpy(synthetic.synthetic_params(3, seed=9)).cuda()
        d = hm.decode(p, to_2d=False, flip_z=True, landmarks=False)
        img = mesh.render(d["proj"], torch.zeros((3, 256, 256, 3), dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        outs.append((d["verts3d"].clone(), img.clone()))
        n = C.c_uint()
        _lib.check(lib.dad3d_flame_handoff_timeouts(hm.flame._handle, C.byref(n)))
        assert n.value == 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert int(outs[0][1].max()) > 0


def _run_bench(cmd, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LOCAL_RANK")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    return p


def test_bench_plain_and_torchrun_lines_agree_and_two_gpus_are_refused():
    """The driver's contract: `python bench.py --gpus 1` and the same under torch.distributed.run (N = 1: RCCL process group,
    warm-up gather, timed all_gather_into_tensor) print one JSON line each that agree within noise; a 20-step run agrees
    with a 2000-step run within 5 %; `--gpus 2` on this 1-GPU box says what is wrong."""
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline", "--no-secondary"]
    plain = _run_bench(base + ["--gpus", "1", "--steps", "2000", "--warmup", "100"])
    assert plain.returncode == 0, plain.stderr[-800:]
    a = json.loads(plain.stdout.strip().splitlines()[-1])
    short = _run_bench(base + ["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert short.returncode == 0, short.stderr[-800:]
    s = json.loads(short.stdout.strip().splitlines()[-1])
    tr = _run_bench([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
                     "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline", "--gpus", "1",
                     "--steps", "2000", "--warmup", "100"])
    assert tr.returncode == 0, tr.stderr[-800:]
    lines = [ln for ln in tr.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # rank 0 prints ONE JSON line
    b = json.loads(lines[0])
    for d in (a, s, b):
        assert d["config"]["outputs_verified"] is True and d["config"]["handoff_timeouts"] == 0 and d["n_gpus"] == 1
        assert d["roofline"]["frac"] > 0.3 and d["unit"] == "images/sec"
        # every line runs the job's one collective behind its K steps and prints both per-step times
        assert d["config"]["gather_via"] is not None and d["ms_per_step_with_gather"] >= d["ms_per_step_compute"] > 0
        # round 6: both definitions of the job's rate at EVERY N (a scaling curve is read on one of them), the gather's share, the toolchain pair
        assert d["value_compute"] >= d["value_with_gather"] > 0 and d["value"] in (d["value_compute"], d["value_with_gather"])
        assert "gather_in_region_us / region" in d["config"]["scaling_note"] and "Unmeasured on N > 1" in d["config"]["scaling_note"]
        assert d["config"]["toolchain"].startswith("built: clang") and "running: HIP runtime" in d["config"]["toolchain"]
    assert a["value"] == a["value_compute"] and b["value"] == b["value_with_gather"]
    assert "compute" in a["config"]["value_definition"] and "with_gather" in b["config"]["value_definition"]
    assert abs(a["ms_per_step"] - a["ms_per_step_compute"]) < 1e-9 and abs(b["ms_per_step"] - b["ms_per_step_with_gather"]) < 1e-9
    assert "nccl" in b["config"]["parallelism"] and "no process group" in a["config"]["parallelism"]
    assert abs(a["value"] - b["value"]) / a["value"] < 0.10, (a["value"], b["value"])
    assert abs(a["value"] - s["value"]) / a["value"] < 0.05, (a["value"], s["value"])
    # the device-side aligned start (a 4-byte ncclAllGather in front of the opening event) costs the region nothing: the driver's
    # own 20-step command under torchrun against the plain 20-step line, compute time to compute time
    tr20 = _run_bench([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
                       "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline", "--gpus", "1",
                       "--steps", "20", "--warmup", "5"])
    assert tr20.returncode == 0, tr20.stderr[-800:]
    c = json.loads([ln for ln in tr20.stdout.strip().splitlines() if ln.startswith("{")][0])
    assert "ncclAllGather" in c["config"]["start_alignment"] and c["config"]["start_skew_us"]["max"] >= c["config"]["start_skew_us"]["min"] >= 0
    assert a["config"]["start_alignment"] == "none" and a["config"]["start_skew_us"] is None
    print("ms_per_step_compute plain-20 / torchrun-20:", s["ms_per_step_compute"], c["ms_per_step_compute"], "skew", c["config"]["start_skew_us"])
    assert abs(c["ms_per_step_compute"] - s["ms_per_step_compute"]) / s["ms_per_step_compute"] < 0.08  # measured: 0.2-2 % (two 0.26 ms regions)
    if torch.cuda.device_count() < 2:
        two = _run_bench(base + ["--gpus", "2", "--steps", "5", "--warmup", "1"], timeout=120)
        assert two.returncode != 0 and "2 GPUs requested, 1 visible" in two.stderr, two.stderr[-500:]


def test_bench_eight_ranks_code_path_on_one_gpu():
    """The N = 8 code path of bench.py before an 8-GPU node ever sees it: eight ranks under torch.distributed.run sharing the one
    GPU (DAD3D_BENCH_SHARE_GPU=1: gloo, host-staged gathers), both workloads -- per-rank seeds, MAX over ranks, the gather of
    8 x 64 rows and its check, the two per-step times, clean teardown. Not a multi-GPU measurement, and the line says so."""
    for workload, steps, extra in (("decode", "100", []), ("render", "20", []), ("render", "20", ["--gather", "all"])):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline", "--gpus", "8", "--steps", steps,
               "--warmup", "10", "--workload", workload] + extra
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LOCAL_RANK")}
        env["DAD3D_BENCH_SHARE_GPU"] = "1"
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-1500:]
        lines = [ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")]
        assert len(lines) == 1  # rank 0 prints ONE JSON line
        d = json.loads(lines[0])
        assert d["n_gpus"] == 8 and d["config"]["global_batch"] == 512 and d["scaling"] == "weak" and d["value"] > 0
        # the aligned start runs (through the hook's host-staged collective here) and the skew it absorbed is printed, MAX and MIN over ranks
        assert "TEST HOOK" in d["config"]["start_alignment"] and d["config"]["start_skew_us"]["max"] >= d["config"]["start_skew_us"]["min"] >= 0
        print(workload, extra, "start_skew_us", d["config"]["start_skew_us"])
        if workload == "render":
            assert d["config"]["gather_mode"] == ("all" if extra else "root")
        if workload == "decode":
            assert d["config"]["outputs_verified"] is True and "not a multi-GPU measurement" in d["config"]["parallelism"]
            assert d["ms_per_step_compute"] > 0 and d["ms_per_step_with_gather"] >= d["ms_per_step_compute"]
            assert "with_gather" in d["config"]["value_definition"]
            assert d["value"] == d["value_with_gather"] and d["value_compute"] >= d["value_with_gather"] > 0  # both at every N
            assert "gather_in_region_us / region" in d["config"]["scaling_note"] and d["config"]["toolchain"].startswith("built: clang")
        else:
            assert d["config"]["gather_verified"] is True and d["config"]["images_with_coverage"] == 1.0


def test_bench_two_ranks_code_path_on_one_gpu():
    """N > 1 has never run on multi-GPU hardware (no such box is available to the builder). What CAN run here: the whole
    N = 2 code path of bench.py -- two ranks under torch.distributed.run, per-rank seeds and buffers, barrier + synchronize
    brackets, MAX over ranks, the final gather of 2 x 64 x 445 landmarks and its check -- with both ranks sharing the one GPU
    and the collective on gloo (RCCL refuses two ranks per device). The line must say that it is not a multi-GPU measurement."""
    env_extra = {"DAD3D_BENCH_SHARE_GPU": "1"}
    for workload, steps in (("decode", "300"), ("render", "60")):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline", "--gpus", "2", "--steps", steps,
               "--warmup", "20", "--workload", workload]
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LOCAL_RANK")}
        env.update(env_extra)
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-1500:]
        lines = [ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 128 and d["scaling"] == "weak"
        if workload == "decode":
            assert d["config"]["outputs_verified"] is True and d["config"]["handoff_timeouts"] == 0
            assert "not a multi-GPU measurement" in d["config"]["parallelism"]
            assert d["value"] == d["value_with_gather"] and d["value_compute"] >= d["value_with_gather"] > 0
            assert "gather_in_region_us / region" in d["config"]["scaling_note"] and "Unmeasured" not in d["config"]["scaling_note"]
        else:
            assert d["config"]["gather_verified"] is True and d["config"]["images_with_coverage"] == 1.0
        assert d["value"] > 0


def test_driver_command_carries_the_secondary_legs():
    """`python bench.py --gpus 1 --steps 20 --warmup 5 --full`: the contract fields as before, plus -- measured in the
    same process after the contract region -- long_region, secondary.decode_b256 (BASELINE configs[2], every row held to
    reference-HeadMesh goldens), secondary.render_b64 (configs[4] per-GPU share, timed images re-rasterised by the reference's own
    C++) and cpu_baseline_render; the whole run inside the driver's budget."""
    import time

    t0 = time.time()
    p = _run_bench([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    took = time.time() - t0
    assert p.returncode == 0, p.stderr[-800:]
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 20 and d["config"]["outputs_verified"] is True and d["roofline"]["frac"] > 0.3 and d["cpu_baseline"]["value"] > 0
    lr, b256, rnd = d["long_region"], d["secondary"]["decode_b256"], d["secondary"]["render_b64"]
    assert lr["steps"] == 2000 and abs(lr["ms_per_step"] - d["ms_per_step"]) / d["ms_per_step"] < 0.10
    assert b256["outputs_verified"] is True and b256["verification"]["rows"] == 256 and 0.4 < b256["frac"] < 1.0 and b256["hbm_frac"] < 1.0
    assert rnd["timed_images_match_reference_raster"] is True and rnd["images_with_coverage"] == 1.0 and rnd["images_per_sec"] > 1e5
    lo = b256["landmarks_only"]
    assert lo["outputs_verified"] is True and lo["sub_model_vertices"] > 400 and lo["images_per_sec"] > 1.5 * b256["images_per_sec"]
    assert lo["landmark_px_differ_from_whole_mesh_launch"] == 0 and 0 < lo["frac"] < 1 and lo["b2048"]["nonzero"] is True  # one arithmetic
    sp = d["secondary"]["decode_b256_split"]  # the gated bf16x3 split: same rows, same goldens, its own fractions; never the headline
    assert sp["outputs_verified"] is True and sp["dtype"].startswith("bf16x3") and 0 < sp["frac_bf16"] < 1 and sp["fp32_equivalent_TFLOPs"] > 0
    assert d["dtype"] == "f32" and "split" not in d["roofline"]["kernel"]
    sf = d["secondary"]["decode_b256_split_f16"]  # its second form: two fp16 planes, three products
    assert sf.get("outputs_verified") is True, sf
    assert sf["verification"]["max_abs_3d"] < 5e-6 and sf["verification"]["max_abs_px"] < 1e-3 and sf["verification"]["landmark_gather_exact"]
    assert sf["ms_per_step"] < 0.030, sf  # measured 0.020-0.021 (the bf16 form 0.025, the fp32 leg 0.038)
    for leg in (sp, sf):  # the contract's own step on the split forms: within the bars of each other and the default kernel
        c64 = leg["contract_step_b64"]
        assert "error" not in c64 and c64["max_abs_3d_vs_default_kernel"] < 1e-6 and c64["max_abs_px_vs_default_kernel"] < 5e-4, c64
    for leg in (sp, sf):  # landmark outputs only on a split handle: its sub-model, its arithmetic
        lo2 = leg["landmarks_only"]
        assert "error" not in lo2 and lo2["bit_equal_to_this_handles_whole_mesh_launch"] is True and lo2["b2048_nonzero"] is True, lo2
    e2e = d["secondary"]["e2e_b64"]  # the north star's sentence, reported separately from the metric
    assert "error" not in e2e, e2e
    assert e2e["gpu_outputs_finite"] is True and e2e["cpu_reference_predictor"]["threads"] == 8 and e2e["ratio"] > 0 and e2e["north_star_target_ratio"] == 200
    assert rnd["two_streams"]["images_per_sec"] > 0.9 * rnd["images_per_sec"]  # two batches in flight: never meaningfully slower than one
    assert d["cpu_baseline_render"]["value"] > 0 and d["cpu_baseline_render"]["cores"] == 1
    assert d["secondary"]["outputs_verified"] is True
    print(f"driver command took {took:.0f} s; long {lr['ms_per_step'] * 1e3:.2f} us, b256 {b256['ms_per_step'] * 1e3:.2f} us frac {b256['frac']:.3f}, "
          f"render {rnd['us_per_batch']:.1f} us")
    assert took < 150  # the driver's run was 32 s in round 4; the secondary legs add ~20 s (two CPU baselines dominate)


def test_plain_bench_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path, static):
    """`python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR`: the headline fields and none of the legs that `--full`
    adds (CPU baselines, secondary legs, the world-1 gather, the golden check); the dumped arrays are float32 and are the last timed
    step's outputs -- rows of the golden's seeded batch within the bars bench.py's own check holds them to, landmark pixels = the
    truncated projection at the 445 indices."""
    from dad_3dheads_amd import landmarks

    p = _run_bench([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                    "--dump-outputs", str(tmp_path)])
    assert p.returncode == 0, p.stderr[-800:]
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["unit"] == "images/sec" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 20
    assert d["metric"].startswith("images/sec (FLAME decode + 445-lmk projection)")
    assert d["value"] == d["value_compute"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 - 64) < 1e-6
    for leg in ("cpu_baseline", "cpu_baseline_render", "long_region", "secondary"):
        assert leg not in d, leg
    assert d["config"]["gather_via"] is None and d["config"]["verification"] is None and d["roofline"]["shader_clock_mhz"] is None
    v, pr, lm = (np.load(tmp_path / f"{k}.npy") for k in ("verts3d", "proj", "lmk_px"))
    assert [a.dtype for a in (v, pr, lm)] == [np.float32] * 3 and v.shape == (64, 5023, 3) and pr.shape == (64, 5023, 2) and lm.shape == (64, 445, 2)
    with np.load(os.path.join(ROOT, "tests", "golden", "decode_golden.npz")) as g:
        sub = g["b64_subset"]
        assert np.abs(v[:, sub] - g["b64_v3d_sub"]).max() < 5e-6 and np.abs(pr[:, sub] - g["b64_proj_sub"]).max() < 1e-3
    idx = landmarks.canonical("445", static)
    assert np.array_equal(lm, pr[:, idx].astype(np.int32).astype(np.float32))
