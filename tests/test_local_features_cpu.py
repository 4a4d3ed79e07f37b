"""CPU side of the local point-distribution features: the fp64 reference (tests/local_features_ref.py) on hand-computed
neighbourhoods, the parameter surgery of lpdnet_hip.features.convert_to_local_features, the wrapper's checkpoint round trip and the
no-fallback rule.  The kernel itself is tested on the GPU (tests/test_local_features_gpu.py)."""
import inspect
import math

import numpy as np
import pytest
import torch

import local_features_ref as R
from oracle import lpd_oracle as orc


def _one(points, k=None):
    """features of point 0 of a single cloud whose list is 0 .. n-1 in the given order"""
    p = np.asarray(points, dtype=np.float32)[None]
    idx = np.arange(p.shape[1], dtype=np.int32)[None, None, :].repeat(p.shape[1], axis=1)
    f, gap = R.features(p, idx, k=k)
    return f[0, 0], gap[0, 0]


def test_reference_on_a_line():
    t = np.arange(8, dtype=np.float64)
    f, _ = _one(np.stack((t, 2 * t, -t), axis=1) * 0.25)
    assert abs(f[2] - 1.0) < 1e-12 and abs(f[0]) < 1e-12 and abs(f[3]) < 1e-9      # L = 1, C = 0, A = 0
    assert abs(f[7] - 7 * 0.25) < 1e-12                                            # dZ: the line spans 7 steps of -0.25 in z


def test_reference_on_the_axis_neighbours_of_a_lattice_point():
    pts = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f, _ = _one(pts)
    # S = (2/7) I: e = 1/3 each
    assert abs(f[0] - 1 / 3) < 1e-12 and abs(f[1] - 1 / 3) < 1e-12 and abs(f[3] - math.log(3)) < 1e-12
    assert abs(f[2]) < 1e-12 and abs(f[6] - 1.0) < 1e-12                           # isotropic: L = 0, L2 = 1
    assert abs(f[5] - 4 / 7) < 1e-12 and abs(f[8] - 2 / 7) < 1e-12 and abs(f[7] - 2.0) < 1e-12
    assert abs(f[9] - 7 / (4 / 3 * math.pi)) < 1e-9                                # r = 1


def test_reference_on_a_planar_patch():
    gx, gy = np.meshgrid(np.arange(3), np.arange(3))
    f, gap = _one(np.stack((gx.ravel(), gy.ravel(), 0 * gx.ravel()), axis=1))
    assert abs(f[0]) < 1e-12 and abs(f[4] - 1.0) < 1e-12 and gap > 0.5             # C = 0, V = 1
    assert f[7] == 0 and f[8] == 0
    same, _ = _one(np.ones((5, 3)))
    assert (same == 0).all()                                                       # no extent: every column 0


def test_reference_sizes_and_test_clouds():
    x = R.clouds(4, 256, seed=1)
    assert x.dtype == np.float32 and x.shape == (4, 256, 3) and np.abs(x).max() <= 1.1
    assert np.array_equal(x, R.clouds(4, 256, seed=1))
    idx = R.knn_lists(x, 12)
    assert (idx[:, :, 0] == np.arange(256)).all()                                  # self first
    kopt = np.where(np.arange(256) % 2 == 0, 8, 12)[None].repeat(4, axis=0)
    f, _ = R.features(x, idx, kopt=kopt)
    f8, _ = R.features(x, idx, k=8)
    f12, _ = R.features(x, idx, k=12)
    assert np.array_equal(f[:, 0::2], f8[:, 0::2]) and np.array_equal(f[:, 1::2], f12[:, 1::2])
    E = R.entropies(x, idx, (8, 12))
    assert np.array_equal(E[..., 0], f8[..., 3]) and np.array_equal(E[..., 1], f12[..., 3])
    assert (f8[..., :5] >= 0).all() and (f8[..., :5] <= math.log(3) + 1e-12).all() # the scale-free columns live in [0, ln 3]


def test_public_surface_and_no_cpu_fallback():
    from lpdnet_hip import LpdHipError, _lib, features, ops
    assert len(features.COLUMNS) == 10 and features.DEFAULT_COLUMNS == (0, 1, 2, 3, 4)
    assert "lpd_local_features" in _lib.SIGNATURES and len(_lib.SIGNATURES["lpd_local_features"]) == 14
    sig = inspect.signature(ops.local_features)
    assert [p for p in sig.parameters] == ["xyz_rows", "idx", "B", "N", "candidates", "columns", "copy_xyz", "want_k", "out"]
    with pytest.raises(LpdHipError):
        features.local_features(torch.zeros(1, 64, 3))
    with pytest.raises(LpdHipError):
        features.append_local_features(torch.zeros(1, 1, 64, 3))
    with pytest.raises(LpdHipError):
        ops.local_features(torch.zeros(64, 3), torch.zeros(1, 64, 8, dtype=torch.int32), 1, 64)
    with pytest.raises(ValueError):
        features.local_features(torch.zeros(1, 64, 8))
    src = open(features.__file__).read()
    assert "import oracle" not in src and "from oracle" not in src


@pytest.mark.parametrize("featnet,kw", [("lpdnet", {}), ("lpdnetorigin", {}), ("lpdnet", dict(xyz_trans=True, feature_transform=True))])
def test_convert_to_local_features(featnet, kw):
    from lpdnet_hip import features
    from util.PointNetVlad import PointNetVlad
    m = PointNetVlad(num_points=256, featnet=featnet, **kw)
    m.load_state_dict(orc.synthetic_state(featnet, num_points=256, **kw), strict=True)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    old = m.emb_nn
    old_ptrs = {k: v.data_ptr() for k, v in old.state_dict().items()}
    assert features.convert_to_local_features(m) is m
    new = m.emb_nn
    assert type(new) is type(old) and new is not old and new.use_mFea
    assert (new.t3d, new.tfea, new.use_relu, new.k, new.emb_dims) == (old.t3d, old.tfea, old.use_relu, old.k, old.emb_dims)
    after = m.state_dict()
    want = orc.state_shapes(featnet, num_points=256, use_mFea=True, **kw)
    assert {k: tuple(v.shape) for k, v in after.items()} == {k: tuple(v) for k, v in want.items()}
    key = "emb_nn." + features._conv1_key(new)
    assert tuple(after[key].shape) == (64, 8, 1)
    assert torch.equal(after[key][:, :3], before[key]) and (after[key][:, 3:] == 0).all()
    for k, v in after.items():
        if k != key:
            assert torch.equal(v, before[k]), k
    assert all(v.data_ptr() != old_ptrs[k] for k, v in new.state_dict().items())      # every tensor is a copy
    assert features.convert_to_local_features(m).emb_nn is new                     # already converted: nothing to do
    with pytest.raises(ValueError):
        features.convert_to_local_features(PointNetVlad(num_points=256, featnet="pointnet"))


def test_wrapper_checkpoint_round_trip(tmp_path):
    from lpdnet_hip import features, harness
    from util.PointNetVlad import PointNetVlad
    m = features.convert_to_local_features(PointNetVlad(num_points=256, featnet="lpdnet"))
    m.load_state_dict(orc.synthetic_state("lpdnet", num_points=256, use_mFea=True), strict=True)
    w = features.LocalFeatureInput(m, k=16, candidates=(8, 16))
    assert w.module is m and harness._unwrap(w) is m and list(w.parameters())[0] is list(m.parameters())[0]
    assert all(k.startswith("module.") for k in w.state_dict())
    opt = torch.optim.SGD(w.parameters(), lr=0.1)
    path = str(tmp_path / "model.ckpt")
    harness.save_checkpoint(path, w, opt, 3, 17, 0.5)
    blob = torch.load(path, map_location="cpu", weights_only=False)
    assert set(blob["state_dict"]) == set(m.state_dict())                          # the unwrapped model's keys
    m2 = features.convert_to_local_features(PointNetVlad(num_points=256, featnet="lpdnet"))
    w2 = features.LocalFeatureInput(m2)
    assert harness.load_pretrained(w2, path) == (4, 17)
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    w.train()
    assert m.training and m.emb_nn.training
    w.eval()
    assert not m.training
