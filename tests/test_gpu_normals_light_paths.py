"""GPU: the vertex normals and the Phong light on EVERY kernel form the launchers can choose, against the compiled reference
(normals, bit for bit) and a float64 restatement of Sim3DR/lighting.py (light).

`launch_get_normal` / `launch_phong` pick among a face-normal-table kernel at 1, 2, 4 or 8 vertex chunks per image, a
staged-LDS gather and a global-memory gather, from the mesh size and from CUs / batch; `Mesh.render` lights inside the
raster's geometry kernel through a table or a gather. `Mesh.normal_plan` reports that decision from the launchers' own
functions, and `test_sweep_reaches_every_form` proves through it that the meshes and batches below reach every form, so
the sweep cannot silently shrink. The meshes are the smallest that reach a branch:

  tiny_N          N = 1, 2, 3, 7, 8, 9 vertices: fewer vertices than chunks (empty chunks), zero-area and repeated-corner faces
  valence         hubs of degree exactly 7, 8, 9 and 40 (the 0xFFFE "more than eight faces" tail of row8), vertices in no face,
                  a face listed twice, a face with one vertex in two corners
  stage_rest_N    N = 5461, 5462, 5463: around the 4096 float4 the staging requests ahead; its rest loop runs at 5463
  face_loop       a one-chunk table of more than kFacesAhead * 1024 = 4096 faces: the rest loop of the face pass
  partial         only the 4- and 8-chunk tables fit the LDS
  lds_only        no table fits, the vertices do: the staged gather
  phong_refused_N N = 13566, 13650: get_normal stages, phong_light must refuse on the host
  global_N        N = 13651 and 70000 (> 65535: no 16-bit face lists at all): the global gather

Every image of a batch is different: image b takes vertex profile b mod 7 (plain, pixel-centre integers, flat with -0.0,
1e7 outliers, 1e-8 scale, 3e38 outliers, 1e-19 scale) and its own random stream. Batches: 1, 3 and, for q in 8, 5, 4, 3, 2,
CUs // q and the batch after it (every value at which min(8, CUs // batch) or the table chunking changes), all from the
device's CU count. The large meshes take batch 1 and the first batch with one chunk.

Light tolerance (`lighting_restatement.light_error_report`): 2e-5 against float64, or four times numpy-float32's own distance
from float64 where that exceeds 5e-6; vertices whose float64 cos is nonzero below 1e-6 are left out (< 1 % asserted), the
`cos != 0` gate of lighting.py:60 being undecided there in float32. The light is compared on the five profiles that keep
float32 finite; on all seven it must be finite, in [0, 1] and the same bits in all three modes and in `render`.

Measured on an MI355X over this whole module (max |light - float64| over the kept vertices): MEASURED below.
"""
import numpy as np
import pytest
import torch

from dad_3dheads_amd._lib import Dad3dError
from dad_3dheads_amd.Sim3DR import Mesh
from lighting_restatement import light_error_report, phong_light_f64
from oracle.sim3dr_ref import phong_light_ref

pytestmark = pytest.mark.gpu

# max |kernel - float64| / max |numpy float32 - float64| over the kept vertices, per group of cases (MI355X, 256 CUs):
MEASURED = """
  cases (every batch and configuration)   kernel    numpy float32   left out of kept vertices
  tiny_1 .. tiny_9                        1.07e-6   9.9e-7          14 of 4.5e3 at most (tiny_8)
  valence                                 2.95e-6   2.95e-6         0 of 1.7e5
  stage_rest_5461 / 5462 / 5463           2.17e-6   2.15e-6         93 of 3.1e6 at most
  face_loop                               2.19e-6   2.19e-6         6 of 1.7e6
  partial                                 1.65e-6   1.59e-6         0 of 1.5e6
  lds_only                                1.76e-6   1.67e-6         6 of 2.2e6
  the FLAME head, exponent 5 / 64         1.5e-7 / 1.12e-6   1.5e-7 / 1.15e-6   (kernel and numpy 6e-8 / 9e-8 apart)
numpy float32 never left the quiet 5e-6, so every case was held to 2e-5; the kernel is no further from float64 than numpy is:
the 2e-5 covers float32 rounding of the whole formula, of which pow is a small part.
"""
__doc__ += MEASURED

H, W = 48, 64  # the image `render` draws into: one tile
POISON = 7.7e33
PROFILES = ("plain", "pixel_centres", "flat", "wild7", "small", "wild38", "tiny")
BENIGN = 5  # the first five keep float32 finite and the normals unit or exactly zero: the light is compared on them

CONFIGS = {
    "default": {},
    "ambient_only": dict(ambient=0.45, directional=0.0, specular=0.0, color_ambient=(0.2, 0.9, 0.5)),
    "specular_without_directional": dict(ambient=0.2, directional=0.0, specular=0.7),  # lighting.py:47: the specular term sits inside
    "no_specular": dict(specular=0.0),
    "gates_negative": dict(ambient=-0.2, directional=0.7, specular=0.3),
    "colours": dict(color_ambient=(0.9, 0.3, 0.1), color_directional=(0.2, 0.7, 1.0)),
    "clipped_sum": dict(ambient=0.5, directional=0.8, specular=0.9, color_directional=(1.0, 0.6, 0.3)),
    "off_axis": dict(light_pos=(3.0, -2.0, 1.5), view_pos=(-1.0, 4.0, 2.5)),
    **{f"exp_{e}": dict(specular_exp=e, specular=0.4, light_pos=(1.0, 2.0, 4.0)) for e in (0, 1, 2, 3, 4, 5, 63, 64, 65, 2.5)},
}
ROTATION = ("default", "colours", "off_axis", "clipped_sum", "exp_3", "exp_64", "exp_65", "exp_2.5")  # one per batch in the batch sweep


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def sweep_batches():
    cus = _cus()
    return sorted({1, 3} | {b for q in (8, 5, 4, 3, 2) for b in (max(1, cus // q), cus // q + 1)})


def one_chunk_batch():
    return _cus() // 2 + 1  # the first batch with min(8, CUs // batch) == 1


# ------------------------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------------------------
def grid_triangles(nver, cols, both):
    """Vertex i at column i % cols, row i // cols; one (or both) triangle(s) per cell whose corners exist; faces in
    vertex order, so spatially sorted."""
    i = np.arange(nver)
    ok = (i % cols != cols - 1) & (i + cols < nver)
    a = i[ok]
    t = np.stack([a, a + 1, a + cols], 1)
    if both:
        b = i[ok & (i + cols + 1 < nver)]
        t = np.concatenate([t, np.stack([b + 1, b + cols + 1, b + cols], 1)])
        t = t[np.argsort(t.min(1), kind="stable")]
    return np.ascontiguousarray(t, np.int32)


def tiny_triangles(nver):
    rng = np.random.default_rng(100 + nver)
    t = rng.integers(0, nver, (2 * nver + 3, 3))
    extra = [(0, 0, 0), (nver - 1, 0, nver - 1)]  # repeated corners
    if nver >= 3:
        extra.append((0, 1, 2))  # vertices 1 and 2 share a position (image_vertices): zero area, three different corners
    return np.ascontiguousarray(np.concatenate([t, np.array(extra)]), np.int32)


def valence_triangles():
    rng = np.random.default_rng(5)
    tris, nxt = [], 4
    for hub, deg in ((0, 7), (1, 8), (2, 9), (3, 40)):  # a fan of `deg` faces around the hub over deg + 1 rim vertices
        rim = np.arange(nxt, nxt + deg + 1)
        nxt += deg + 1
        tris += [(hub, rim[k], rim[k + 1]) for k in range(deg)]
    assert nxt == 72  # 72 .. 89 stay in no face
    tris += [tuple(r) for r in rng.choice(np.arange(90, 300), (380, 3))]
    tris += [(90, 91, 92), (90, 91, 92), (93, 93, 94)]  # listed twice; one vertex in two corners
    t = np.array(tris, np.int32)
    return np.ascontiguousarray(t[rng.permutation(len(t))])


MESHES = {  # name -> (nver, triangles builder, large)
    **{f"tiny_{n}": (n, lambda n=n: tiny_triangles(n), False) for n in (1, 2, 3, 7, 8, 9)},
    "valence": (300, valence_triangles, False),
    **{f"stage_rest_{n}": (n, lambda n=n: grid_triangles(n, 128, False), False) for n in (5461, 5462, 5463)},
    "face_loop": (3000, lambda: grid_triangles(3000, 60, True), False),
    "partial": (9000, lambda: grid_triangles(9000, 100, False), True),
    "lds_only": (13000, lambda: grid_triangles(13000, 60, True)[:20000], True),
    **{f"phong_refused_{n}": (n, lambda n=n: grid_triangles(n, 150, False), True) for n in (13566, 13650)},
    "global_13651": (13651, lambda: grid_triangles(13651, 150, False), True),
    "global_70000": (70000, lambda: grid_triangles(70000, 250, True), True),
}


def image_vertices(name, nver, tri, b):
    """Image b of mesh `name`: a bumpy sheet over the index grid (the grid meshes' faces are its cells; the other meshes
    just take scattered points), then the profile b mod 7."""
    rng = np.random.default_rng([sum(map(ord, name)), nver, b])
    profile = PROFILES[b % len(PROFILES)]
    v = np.empty((nver, 3), np.float64)
    if name.startswith(("tiny", "valence")):
        v[:, 0], v[:, 1], v[:, 2] = rng.uniform(-12, W + 12, nver), rng.uniform(-12, H + 12, nver), rng.uniform(-4, 4, nver)
    else:
        cols = int(tri[0, 2] - tri[0, 0])  # the grid's row length
        i = np.arange(nver)
        rows = (nver + cols - 1) // cols
        x, y = (i % cols) / cols, (i // cols) / rows
        v[:, 0] = -8 + (W + 16) * x + rng.uniform(-0.2, 0.2, nver)
        v[:, 1] = -8 + (H + 16) * y + rng.uniform(-0.2, 0.2, nver)
        v[:, 2] = 6 * np.sin(5 * x + b) * np.cos(4 * y - b) + rng.uniform(-0.3, 0.3, nver)
    if profile == "pixel_centres":  # integer x and y, half-integer depths
        v[:, :2] = np.round(v[:, :2] * 8)
        v[:, 2] = np.round(v[:, 2] * 2) / 2
    elif profile == "flat":  # a plane: every normal is +-z or zero; half of the depths are -0.0
        v[:, 2] = np.where(rng.random(nver) < 0.5, -0.0, 0.0)
    elif profile == "wild7":
        v[rng.integers(0, nver, 3), rng.integers(0, 3, 3)] = rng.choice([1e7, -1e7, 65535.5], 3)
    elif profile == "small":
        v *= 1e-8
    elif profile == "wild38":  # float32 overflows: inf and NaN normals, which the kernels must reproduce
        v[rng.integers(0, nver, 3), 0] = rng.choice([1e7, -1e7, 3e38, -3e38, 65535.5], 3)
        v[rng.integers(0, nver, 2), 1] = rng.choice([1e7, -3e38], 2)
        v[rng.integers(0, nver, 2), 2] = rng.choice([3e38, -3e38, 1e-40], 2)
    elif profile == "tiny":  # cross products around 1e-38: denormals, squared lengths that underflow to the `len <= 0` branch
        v *= 1e-19
    v = v.astype(np.float32)
    if profile == "plain" and nver > 3:
        v[rng.integers(0, nver)] = (-0.0, 0.0, -0.0)
    if name.startswith("tiny") and nver >= 3:
        v[2] = v[1]
    return np.ascontiguousarray(v)


def prefill(nver, b):
    """What `accumulate=True` adds onto: ordinary values, rows of -0.0, huge rows and NaN rows."""
    rng = np.random.default_rng([nver, b, 17])
    p = rng.normal(0, 3, (nver, 3)).astype(np.float32)
    r = np.arange(nver)
    p[r % 11 == 0] = -0.0
    p[r % 11 == 7] = np.float32(1e30) * np.sign(p[r % 11 == 7])
    p[r % 11 == 5] = np.nan
    p[r % 11 == 9, 1] = 3e38
    return p


class Case:
    def __init__(self, name):
        self.name = name
        self.nver, build, self.large = MESHES[name]
        self.tri = build()
        self.ntri = len(self.tri)
        self.mesh = Mesh(self.tri, self.nver, device=0)
        self.batches = [1, one_chunk_batch()] if self.large else sweep_batches()
        self._v, self._n = [], []
        self.stats = dict(gpu=0.0, np32=0.0, kept=0, left_out=0)

    def verts(self, batch):
        while len(self._v) < batch:
            self._v.append(image_vertices(self.name, self.nver, self.tri, len(self._v)))
        return self._v[:batch]

    def normals(self, oracle, batch):  # the reference's, computed once per image and shared by every test of the case
        v = self.verts(batch)
        while len(self._n) < batch:
            self._n.append(oracle.get_normal(v[len(self._n)], self.tri))
        return self._n[:batch]

    def dev(self, batch):
        return torch.from_numpy(np.stack(self.verts(batch))).cuda()

    def plan(self, entry, batch=1):
        return self.mesh.normal_plan(batch, entry, H, W)


_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(scope="module", autouse=True)
def release_cases():
    yield
    _CASES.clear()  # the mesh handles and their device memory go with the module


@pytest.fixture(scope="module", params=list(MESHES))
def case(request):
    c = get_case(request.param)
    yield c
    c._v, c._n = [], []  # the large meshes hold a few hundred MB of images


def framed(batch, rows):
    """[batch, rows, 3] inside a poisoned buffer with one image of margin on either side."""
    big = torch.full((batch + 2, rows, 3), POISON, dtype=torch.float32, device="cuda")
    return big, big[1:-1]


def margins_intact(big):
    return bool((big[0] == POISON).all() and (big[-1] == POISON).all())


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------
# the sweep reaches every form
# ------------------------------------------------------------------------------------------------------------------
def test_sweep_reaches_every_form():
    cus = _cus()
    reached = {"get_normal": set(), "phong_light": set(), "render": set()}
    for name in MESHES:
        c = get_case(name)
        for entry in ("get_normal", "phong_light"):
            for b in c.batches:
                p = c.plan(entry, b)
                reached[entry].add((p["form"], p["chunks"]) if p["form"] == "table" else p["form"])
                assert p["form"] != "table" or p["chunks"] in p["built"]
                if p["form"] in ("table", "lds"):  # the launchers' rule, from the device's CU count
                    want = -(-c.nver // -(-c.nver // max(1, min(8, cus // b))))
                    fits = [k for k in p["built"] if k >= want] or list(p["built"][-1:])
                    assert p["chunks"] == (fits[0] if p["form"] == "table" else want), (name, entry, b, p)
        reached["render"].add(c.plan("render")["form"])
    print("reached:", reached)
    for entry in ("get_normal", "phong_light"):
        assert {("table", k) for k in (1, 2, 4, 8)} <= reached[entry], (entry, reached[entry])
        assert "lds" in reached[entry]
    assert "global" in reached["get_normal"] and "refused" in reached["phong_light"]
    assert {"table", "lds", "refused"} <= reached["render"]
    # the meshes are what their names say
    assert get_case("partial").plan("get_normal")["built"] == (4, 8)
    assert get_case("lds_only").plan("get_normal")["built"] == () and get_case("lds_only").plan("render")["form"] == "lds"
    for n in (5461, 5462, 5463):
        c = get_case(f"stage_rest_{n}")
        assert c.plan("get_normal", one_chunk_batch()) == {"form": "table", "chunks": 1, "built": (1, 2, 4, 8)}
    c = get_case("face_loop")
    assert c.plan("get_normal", one_chunk_batch())["chunks"] == 1 and c.ntri > 4096 and c.plan("render")["form"] == "table"
    for n in (13566, 13650):
        c = get_case(f"phong_refused_{n}")
        assert [c.plan(e, b)["form"] for e in ("get_normal", "phong_light") for b in c.batches] == ["lds", "lds", "refused", "refused"]
    for n in (13651, 70000):
        assert get_case(f"global_{n}").plan("get_normal")["form"] == "global"
    deg = np.bincount(get_case("valence").tri.ravel(), minlength=300)
    assert list(deg[:4]) == [7, 8, 9, 40] and not deg[72:90].any() and deg[93] >= 2
    for n, chunks in ((3, 4), (7, 8), (9, 8)):  # more chunks than ceil(nver / vpb): the launch has empty chunks
        assert get_case(f"tiny_{n}").plan("get_normal", 1) == {"form": "table", "chunks": chunks, "built": (1, 2, 4, 8)}


# ------------------------------------------------------------------------------------------------------------------
# normals: bit for bit
# ------------------------------------------------------------------------------------------------------------------
def test_get_normal_every_batch(case, sim3dr_oracle):
    for b in case.batches:
        ref = case.normals(sim3dr_oracle, b)
        big, out = framed(b, case.nver)
        got = case.mesh.get_normal(case.dev(b), out=out).cpu().numpy()
        assert margins_intact(big), (case.name, b)
        for i in range(b):
            assert np.array_equal(got[i], ref[i], equal_nan=True), (case.name, b, i, PROFILES[i % 7], case.plan("get_normal", b))


def test_get_normal_accumulate(case, sim3dr_oracle):
    for b in sorted({1, 3, case.batches[-1], one_chunk_batch()} & set(case.batches + [3])):
        v = case.verts(b)
        init = [prefill(case.nver, i) for i in range(b)]
        big, out = framed(b, case.nver)
        out.copy_(torch.from_numpy(np.stack(init)))
        got = case.mesh.get_normal(case.dev(b), out=out, accumulate=True).cpu().numpy()
        assert margins_intact(big)
        for i in range(b):
            ref = sim3dr_oracle.get_normal(v[i], case.tri, init=init[i])
            assert np.array_equal(got[i], ref, equal_nan=True), (case.name, b, i, case.plan("get_normal", b))


def test_tri_and_ver_normal(case, sim3dr_oracle):
    b = 3
    v, dv = case.verts(b), case.dev(b)
    for flg in (False, True):
        tn = case.mesh.get_tri_normal(dv, norm_flg=flg)
        tn_h = tn.cpu().numpy()
        big, out = framed(b, case.nver)
        vn = case.mesh.get_ver_normal(tn, out=out).cpu().numpy()
        assert margins_intact(big)
        init = [prefill(case.nver, 40 + i) for i in range(b)]
        big, acc = framed(b, case.nver)
        acc.copy_(torch.from_numpy(np.stack(init)))
        va = case.mesh.get_ver_normal(tn, out=acc, accumulate=True).cpu().numpy()
        assert margins_intact(big)
        for i in range(b):
            ref_t = sim3dr_oracle.get_tri_normal(v[i], case.tri, norm_flg=flg)
            assert np.array_equal(tn_h[i], ref_t, equal_nan=True), (case.name, flg, i)
            assert np.array_equal(vn[i], sim3dr_oracle.get_ver_normal(ref_t, case.tri, case.nver), equal_nan=True), (case.name, flg, i)
            assert np.array_equal(va[i], sim3dr_oracle.get_ver_normal(ref_t, case.tri, case.nver, init=init[i]), equal_nan=True), (case.name, flg, i)


# ------------------------------------------------------------------------------------------------------------------
# light
# ------------------------------------------------------------------------------------------------------------------
def light_all_modes(case, dv, cfg):
    """The light of `dv` in all three modes and in `render`, asserted to be the same bits; the fused normals equal
    get_normal's, render's image equals the raster of that light. Returns (light, normals) as numpy."""
    mesh, b = case.mesh, dv.shape[0]
    normals = mesh.get_normal(dv)
    given = mesh.phong_light(dv, normals, **cfg)
    big, n_out = framed(b, case.nver)
    fused = mesh.phong_light(dv, None, normals_out=n_out, **cfg)
    assert margins_intact(big)
    assert same_bits(fused, given), (case.name, b, "normals given vs computed in the launch")
    assert np.array_equal(n_out.cpu().numpy(), normals.cpu().numpy(), equal_nan=True), (case.name, b, "fused normals")
    if case.plan("render")["form"] != "refused":
        big, l_out = framed(b, case.nver)
        img = mesh.render(dv, torch.zeros((b, H, W, 3), dtype=torch.uint8, device="cuda"), light_out=l_out, **cfg)
        assert margins_intact(big)
        assert same_bits(l_out, fused), (case.name, b, "render's light")
        assert torch.equal(img, mesh.rasterize(dv, fused, torch.zeros((b, H, W, 3), dtype=torch.uint8, device="cuda"))), (case.name, b)
    light = fused.cpu().numpy()
    assert np.isfinite(light).all() and light.min() >= 0.0 and light.max() <= 1.0, (case.name, b)
    return light, normals.cpu().numpy()


def check_against_restatement(case, oracle, batch, cfg_name):
    cfg = CONFIGS[cfg_name]
    light, _ = light_all_modes(case, case.dev(batch), cfg)
    v, n = case.verts(batch), case.normals(oracle, batch)
    for i in range(batch):
        if i % len(PROFILES) >= BENIGN:
            continue
        r = light_error_report(light[i], n[i], v[i], **cfg)
        s = case.stats
        s["gpu"], s["np32"] = max(s["gpu"], r["gpu_err"]), max(s["np32"], r["np32_err"])
        s["kept"], s["left_out"] = s["kept"] + r["kept"], s["left_out"] + r["left_out"]
        assert r["gpu_err"] <= r["tol"], (case.name, batch, i, PROFILES[i % 7], cfg_name, r)
        if cfg.get("specular_exp", 5) in (1, 2):  # np.power is a copy / a square there, and so is the kernel: every bit
            ref32 = phong_light_ref(n[i], v[i], **cfg)
            ok = np.isfinite(ref32).all(1)
            assert np.array_equal(light[i][ok], ref32[ok]), (case.name, batch, i, cfg_name)
    return light


def refused(case):
    return case.plan("phong_light")["form"] == "refused"


def test_light_every_batch(case, sim3dr_oracle):
    """All modes and the restatement at every batch of the sweep, the configuration rotating with the batch."""
    if refused(case):
        for b in case.batches:
            dv = case.dev(b)
            big, n_out = framed(b, case.nver)
            with pytest.raises(Dad3dError, match=f"phong_light: {case.nver} vertices exceed the LDS staging capacity"):
                case.mesh.phong_light(dv, None, normals_out=n_out)
            with pytest.raises(Dad3dError, match="exceed the LDS staging capacity"):
                case.mesh.phong_light(dv, torch.zeros_like(dv))
            torch.cuda.synchronize()
            assert bool((big == POISON).all()), "a refused phong_light launched something"
            if case.plan("render")["form"] == "refused":
                with pytest.raises(Dad3dError, match="render: needs a 3-channel image and a mesh that fits the LDS"):
                    case.mesh.render(dv, torch.zeros((b, H, W, 3), dtype=torch.uint8, device="cuda"), light_out=n_out)
                torch.cuda.synchronize()
                assert bool((big == POISON).all())
        return
    with np.errstate(all="ignore"):
        for k, b in enumerate(case.batches):
            check_against_restatement(case, sim3dr_oracle, b, ROTATION[k % len(ROTATION)])
    s = case.stats
    print(f"LIGHT {case.name}: kernel {s['gpu']:.3e} numpy-f32 {s['np32']:.3e} kept {s['kept']} left out {s['left_out']}")
    assert s["kept"] == 0 or s["left_out"] < 0.01 * (s["kept"] + s["left_out"]), s  # kept == 0: tiny_1, whose norm_vertices is 0/0


def test_light_configurations(case, sim3dr_oracle):
    """Every configuration at batch 3 (plain, pixel-centre and flat image) and at batch 5 for a few (1e7 outliers, 1e-8 scale)."""
    if refused(case):
        return  # test_light_every_batch asserts the refusal
    with np.errstate(all="ignore"):
        for name in CONFIGS:
            check_against_restatement(case, sim3dr_oracle, 3, name)
        for name in ("default", "exp_1", "exp_2", "exp_64", "clipped_sum"):
            check_against_restatement(case, sim3dr_oracle, 5, name)
    s = case.stats
    print(f"LIGHT {case.name}: kernel {s['gpu']:.3e} numpy-f32 {s['np32']:.3e} kept {s['kept']} left out {s['left_out']}")
    assert s["kept"] == 0 or s["left_out"] < 0.01 * (s["kept"] + s["left_out"]), s  # kept == 0: tiny_1, whose norm_vertices is 0/0


@pytest.mark.parametrize("name", ["valence", "face_loop", "lds_only"])
def test_light_where_numpy_is_nan_fractional_exponent(name, sim3dr_oracle):
    """specular_exp = 3.5: a negative base gives NaN in numpy on most vertices, and np.clip keeps it. The kernel's clip01 is
    fminf(fmaxf()), which returns the other operand for a NaN: the specular term contributes nothing there. So the kernel's
    light is the reference's light WITHOUT the specular term wherever the reference's own is NaN."""
    case = get_case(name)
    cfg = dict(specular_exp=3.5, specular=0.5, light_pos=(1.0, 2.0, 4.0))
    with np.errstate(all="ignore"):
        light, _ = light_all_modes(case, case.dev(3), cfg)
        v, n = case.verts(3), case.normals(sim3dr_oracle, 3)
        nan_share = []
        for i in range(3):
            full = phong_light_f64(n[i], v[i], **cfg)
            nan = ~np.isfinite(full).all(1)
            nan_share.append(nan.mean())
            r = light_error_report(light[i], n[i], v[i], mask=nan, **{**cfg, "specular": 0.0})
            assert r["gpu_err"] <= r["tol"], (name, i, r)
            r = light_error_report(light[i], n[i], v[i], **cfg)  # and the reference's own value where it has one
            assert r["gpu_err"] <= r["tol"], (name, i, r)
    print(f"NAN {name}: share of vertices where float64 is NaN {nan_share}")
    assert max(nan_share) > 0.5


def test_light_of_a_collapsed_mesh_and_of_a_vertex_on_the_light(sim3dr_oracle):
    """gmax == 0 (every vertex in one point) makes norm_vertices 0/0; a vertex on light_pos makes its direction 0/0. numpy
    carries the NaN into the light; the kernel's NaN terms contribute nothing: the ambient term alone, exactly."""
    case = get_case("tiny_9")
    cfg = dict(ambient=0.35, color_ambient=(0.5, 1.0, 0.25), directional=0.6, specular=0.3)
    dv = torch.full((2, 9, 3), 3.25, dtype=torch.float32, device="cuda")
    dv[1] = -0.0
    light, _ = light_all_modes(case, dv, cfg)
    want = np.clip(np.float32(0.35) * np.array(cfg["color_ambient"], np.float32), 0, 1)
    assert np.array_equal(light, np.broadcast_to(want, light.shape))
    light, _ = light_all_modes(case, dv, {**cfg, "ambient": 0.0})
    assert not light.any()
    # a cube corner that norm_vertices maps onto (1, 1, 1) exactly: (x - 0) / 4 * 2 - (4 / 4 * 2) / 2
    rng = np.random.default_rng(3)
    v = rng.integers(0, 5, (9, 3)).astype(np.float32)
    v[0], v[1], v[2] = (0, 0, 0), (4, 4, 4), (4, 4, 4)
    cfg = dict(ambient=0.25, directional=0.5, specular=0.25, light_pos=(1.0, 1.0, 1.0), view_pos=(0.0, 0.5, 3.0), color_ambient=(1.0, 0.5, 0.25))
    light, normals = light_all_modes(case, torch.from_numpy(v).cuda()[None], cfg)
    assert np.array_equal(normals[0], sim3dr_oracle.get_normal(v, case.tri), equal_nan=True)
    with np.errstate(all="ignore"):
        full = phong_light_f64(normals[0], v, **cfg)
        on_light = ~np.isfinite(full).all(1)
        assert list(np.flatnonzero(on_light)) == [1, 2]
        want = np.clip(np.float32(0.25) * np.array(cfg["color_ambient"], np.float32), 0, 1)
        assert np.array_equal(light[0][on_light], np.broadcast_to(want, (2, 3)))
        r = light_error_report(light[0], normals[0], v, **cfg)
    assert r["gpu_err"] <= r["tol"] and r["kept"] + r["left_out"] == 7, r
