"""Run the reference's OWN `model_training/head_mesh.py` unmodified  --  TEST INFRASTRUCTURE.

Authoring-container only (needs /root/reference; the GPU box has none). Used by
tests/golden/make_decode_golden.py to generate the committed fixtures and by
tests/test_oracle_flame.py::test_oracle_bitwise_equals_live_reference (auto-skipped when the reference tree is absent).

The reference cannot be imported as-is here: `hydra`, `smplx`, `pytorch_toolbelt`, `omegaconf`,
`coloredlogs`, `cv2`, `skimage` and `fire` are not installed and `static/flame.pkl` is missing. This module holds the only
stand-in helpers (`stand_in`, `bypass_package_init`) and the shared stand-ins (`install_stand_ins`):

    hydra.utils.instantiate        (model_training/model/__init__.py:1)  -> calls the class a config names
    pytorch_toolbelt.utils         (model_training/model/utils.py:12)    -> image_to_tensor: HWC -> CHW
    smplx.utils.{Struct,to_tensor,to_np}  (flame.py:6, model/utils.py:2) -> 3 tiny helpers re-stated
    smplx.lbs.lbs                  (flame.py:5)                          -> oracle.flame_ref.lbs
    smplx.lbs.find_dynamic_lmk_idx_and_bcoords  (data/utils.py, benchmark utils.py) -> the zero-pose case, re-stated
    omegaconf, coloredlogs, cv2, skimage.io, fire                        -> names only, never called

The generators under tests/golden/ register what is theirs alone through the same `stand_in`. The module
patches `model_training.model.flame.get_flame_model` to hand back the seeded synthetic model.
Everything else -- `HeadMesh`, `FLAMELayer`, `FlameParams`, `rot_mat_from_6dof` -- is the reference's
code, byte for byte, executed from where it lies. Nothing is copied into this repository.
"""
from __future__ import annotations

import functools
import importlib
import os
import sys
import types

import numpy as np
import torch

REFERENCE_ROOT = os.environ.get("DAD3D_REFERENCE_ROOT", "/root/reference")


def reference_available() -> bool:
    return os.path.isfile(os.path.join(REFERENCE_ROOT, "model_training", "head_mesh.py"))


def stand_in(name, **attrs):
    """Register an empty module with `attrs` as `sys.modules[name]`, replacing whatever holds that name, and hang it on its parent
    package when that is registered too. Every stand-in of this module and of the generators under tests/golden/ is made here."""
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    return m


def bypass_package_init(package):
    """Register the reference package `package` (`model_training.data`, ...) as an empty package over its own directory: its
    sub-modules import from where they lie, its `__init__` (which pulls in more uninstalled imports) never runs."""
    return stand_in(package, __path__=[os.path.join(REFERENCE_ROOT, *package.split("."))])


class Struct:
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def _to_tensor(array, dtype=torch.float32):
    return (array if torch.is_tensor(array) else torch.tensor(array)).to(dtype)


def _to_np(array, dtype=np.float32):
    if "scipy.sparse" in str(type(array)):
        array = array.todense()
    return np.array(array, dtype=dtype)


def find_dynamic_lmk_idx_and_bcoords(vertices, pose, dynamic_lmk_faces_idx, dynamic_lmk_b_coords, neck_kin_chain, dtype=torch.float32):
    """`smplx.lbs.find_dynamic_lmk_idx_and_bcoords` for the only way the reference calls it: a ZERO pose. Every rotation of the
    neck chain is then the identity, the yaw angle is 0 and the function returns row 0 of the contour tables (smplx 0.1.26,
    lbs.py: `y_rot_angle = round(clamp(-yaw * 180 / pi, max=39))`, negative angles remapped, then `index_select(table, 0,
    y_rot_angle)`). PARITY UNPINNED for this one function, like `smplx.lbs.lbs` (see oracle/flame_ref.py)."""
    assert float(pose.abs().max()) == 0.0, "the stand-in covers the reference's only call: a zero pose"
    y_rot_angle = torch.zeros(vertices.shape[0], dtype=torch.long)
    return torch.index_select(dynamic_lmk_faces_idx, 0, y_rot_angle), torch.index_select(dynamic_lmk_b_coords, 0, y_rot_angle)


def _instantiate(cfg, *args):
    """`hydra.utils.instantiate` for a config that names a class: `cfg["_target_"]`, imported and called with `args`."""
    module, _, name = cfg["_target_"].rpartition(".")
    return getattr(importlib.import_module(module), name)(*args)


@functools.lru_cache(maxsize=None)
def install_stand_ins():
    """The stand-ins every path through the reference shares, each defined here once with all the attributes any of its users
    reads. Installed by name, whatever held the name before, once per process: what a generator registers afterwards through
    `stand_in` (a `cv2` that serves its seeded images, say) is not undone by a later `load_reference_*` call."""
    from . import flame_ref

    stand_in("smplx")
    stand_in("smplx.utils", Struct=Struct, to_tensor=_to_tensor, to_np=_to_np)
    stand_in("smplx.lbs", lbs=lambda *a, **k: flame_ref.lbs(*a, **k), find_dynamic_lmk_idx_and_bcoords=find_dynamic_lmk_idx_and_bcoords)
    stand_in("hydra")
    stand_in("hydra.utils", instantiate=_instantiate, get_original_cwd=os.getcwd)
    stand_in("pytorch_toolbelt")
    stand_in("pytorch_toolbelt.modules")  # imported by layers.py:8, used only by heads no model here builds
    stand_in("pytorch_toolbelt.utils", image_to_tensor=lambda img: torch.from_numpy(np.ascontiguousarray(np.moveaxis(img, -1, 0))))
    stand_in("omegaconf", OmegaConf=type("OmegaConf", (), {}), DictConfig=dict, ListConfig=list)
    stand_in("coloredlogs", DEFAULT_FIELD_STYLES={}, DEFAULT_LEVEL_STYLES={}, install=lambda *a, **k: None)
    stand_in("cv2")
    stand_in("skimage")
    stand_in("skimage.io", imread=None)
    stand_in("fire", Fire=lambda *a, **k: None)


def load_reference_head_mesh(model, flame_config=None, image_size: int = 256):
    """Return an instance of the reference's HeadMesh driven by `model` (a FLAME-shaped namespace)."""
    if not reference_available():
        raise FileNotFoundError(f"reference tree not found at {REFERENCE_ROOT}")
    sys.dont_write_bytecode = True  # the reference tree is read-only
    install_stand_ins()
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    import model_training.model.flame as ref_flame  # noqa: E402  (reference code)
    from model_training.head_mesh import HeadMesh  # noqa: E402  (reference code)

    fields = {k: getattr(model, k) for k in ("f", "v_template", "shapedirs", "posedirs", "J_regressor", "kintree_table", "weights")}
    ref_flame.get_flame_model = lambda flame_path=None: Struct(**fields)
    with torch.no_grad():
        return HeadMesh(flame_config=flame_config, image_size=image_size)


def load_reference_losses(model):
    """The reference's own `Vertices3DLoss` / `ReprojectionLoss` classes (model_training/losses/*.py, unmodified),
    wired to `model` like `load_reference_head_mesh`. The package `__init__` (which pulls in unrelated losses with more
    uninstalled imports) is bypassed; `model_training/utils.py` finds the stand-ins for `omegaconf`, `coloredlogs` and
    `hydra.utils.get_original_cwd`, none of which the loss path calls."""
    load_reference_head_mesh(model)  # stand-ins, sys.path and the patched get_flame_model
    bypass_package_init("model_training.losses")
    v3d = importlib.import_module("model_training.losses.vertices_3d_loss")
    rep = importlib.import_module("model_training.losses.reprojection_loss")
    return v3d.Vertices3DLoss, rep.ReprojectionLoss


def _pytorchcv_resnet50_features():
    """Stand-in for `pytorchcv.model_provider.get_model("resnet50").features` (encoders.py:5,22; the package is not
    installed here, pinned by the reference's requirements as a third-party dependency): a module tree with pytorchcv's
    published resnet50 layout and NAMES -- `init_block.conv.{conv,bn}`, `stage{1..4}.unit{k}.body.conv{1,2,3}.{conv,bn}`,
    `unit1.identity_conv.{conv,bn}`, stride on conv1 of a unit's bottleneck (`conv1_stride=True`) -- written from the
    architecture, random-initialised. It exists so that the reference's own FlameRegression / BiFPN / heads can be
    executed and so that a state dict with the checkpoint's key names exists; it pins nothing about pytorchcv itself."""
    from torch import nn

    class ConvBlock(nn.Module):
        def __init__(self, cin, cout, k, stride=1, activ=True):
            super().__init__()
            self.conv = nn.Conv2d(cin, cout, k, stride, k // 2, bias=False)
            self.bn = nn.BatchNorm2d(cout)
            self.activ = nn.ReLU(inplace=True) if activ else None

        def forward(self, x):
            x = self.bn(self.conv(x))
            return x if self.activ is None else self.activ(x)

    class ResBottleneck(nn.Module):
        def __init__(self, cin, cout, stride):
            super().__init__()
            mid = cout // 4
            self.conv1 = ConvBlock(cin, mid, 1, stride)
            self.conv2 = ConvBlock(mid, mid, 3)
            self.conv3 = ConvBlock(mid, cout, 1, activ=False)

        def forward(self, x):
            return self.conv3(self.conv2(self.conv1(x)))

    class ResUnit(nn.Module):
        def __init__(self, cin, cout, stride):
            super().__init__()
            self.resize_identity = cin != cout or stride != 1
            self.body = ResBottleneck(cin, cout, stride)
            if self.resize_identity:
                self.identity_conv = ConvBlock(cin, cout, 1, stride, activ=False)
            self.activ = nn.ReLU(inplace=True)

        def forward(self, x):
            identity = self.identity_conv(x) if self.resize_identity else x
            return self.activ(self.body(x) + identity)

    class ResInitBlock(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = ConvBlock(3, 64, 7, 2)
            self.pool = nn.MaxPool2d(3, 2, 1)

        def forward(self, x):
            return self.pool(self.conv(x))

    features = nn.Sequential()
    features.add_module("init_block", ResInitBlock())
    cin = 64
    for i, (cout, units) in enumerate(((256, 3), (512, 4), (1024, 6), (2048, 3))):
        stage = nn.Sequential()
        for j in range(units):
            stage.add_module(f"unit{j + 1}", ResUnit(cin, cout, 2 if (j == 0 and i != 0) else 1))
            cin = cout
        features.add_module(f"stage{i + 1}", stage)
    return features


def load_reference_regressor(seed: int = 0, num_classes: int = 68):
    """The reference's own `FlameRegression` (model_training/model/flame_regression.py:62-105, with its bifpn.py,
    layers.py and encoders.py, unmodified) on the resnet50 configuration of config/model/resnet_regression.yaml,
    random-initialised from `seed`. Stand-ins: `pytorchcv.model_provider.get_model` (see above),
    `pytorch_toolbelt.modules` (imported by layers.py:8, used only by heads this model does not build), `hydra`."""
    if not reference_available():
        raise FileNotFoundError(f"reference tree not found at {REFERENCE_ROOT}")
    sys.dont_write_bytecode = True
    install_stand_ins()
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)

    def get_model(name, pretrained=False, **kwargs):
        if name != "resnet50":
            raise ValueError(f"stand-in only declares resnet50, not {name}")
        return types.SimpleNamespace(features=_pytorchcv_resnet50_features())

    stand_in("pytorchcv")
    stand_in("pytorchcv.model_provider", get_model=get_model)
    bypass_package_init("model_training.data")  # its __init__ pulls in the datasets (albumentations): only data/config.py is needed
    from model_training.model.flame_regression import FlameRegression  # noqa: E402  (reference code)

    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        cfg = {"backbone": "resnet50", "pretrained": False, "num_filters": 256, "num_channels": 3,
               "num_classes": num_classes, "img_size": 256, "conv_block": "regular", "limit_value": 3}
        return FlameRegression(cfg, {}, num_classes=num_classes)
    finally:
        torch.random.set_rng_state(state)
