"""Local point-distribution features on the device: the handcrafted per-point columns of LPD-Net's `use_mFea` trunks.

The reference's LPDNet / LPDNetOrign(use_mFea=True) take [B,1,N,8] inputs = xyz + five per-point features and read those five from
an offline preprocessing step that is not part of the reference (lpdnet_model.py:183-186,215-224).  Here they come from each point's
own neighbourhood in one kernel launch (csrc/lpd_feat.hip; the definition of the ten columns is in include/lpd_hip.h):

    feats = features.local_features(x)                         # [B,N,10] in the caller's point order
    x8 = features.append_local_features(x)                     # [B,1,N,3] -> [B,1,N,8], what a use_mFea trunk takes
    model = features.convert_to_local_features(model)          # an xyz-only PointNetVlad -> the same model with an 8-column conv1
    model = features.LocalFeatureInput(model)                  # [B,1,N,3] clouds in, features computed on the way

The reference does not record which five columns its authors fed, so the selection is a parameter; the default is the five
scale-free ones.  No CPU fallback: inputs must live on the GPU.
"""
import torch
import torch.nn as nn

from . import engine, ops

COLUMNS = ("change_of_curvature", "omnivariance", "linearity", "eigenentropy", "verticality",
           "scattering_2d", "linearity_2d", "height_range", "height_variance", "density")
DEFAULT_COLUMNS = (0, 1, 2, 3, 4)      # the scale-free ones, all in [0, ln 3]


def _cloud_rows(x):
    """[B,N,3] or [B,1,N,3] -> (fp32 rows [B*N,3], B, N)"""
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4) or x.shape[-1] != 3 or (x.dim() == 4 and x.shape[1] != 1):
        raise ValueError(f"expected clouds [B,N,3] or [B,1,N,3], got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
    if not x.is_cuda:
        raise ops._lib.LpdHipError(f"input is on {x.device}: the local features are computed on MI355X only (no CPU fallback)")
    B, N = x.shape[0], x.shape[-2]
    return x.float().contiguous().view(B * N, 3), B, N


def _list_length(k, candidates):
    return max(candidates) if candidates else k


def local_features(x, k=20, candidates=None, columns=range(10)):
    """x [B,N,3] or [B,1,N,3] -> [B,N,len(columns)] in the caller's point order: the xyz kNN with K = max(candidates) if candidates
    else k, then the feature kernel (ops.knn_pm + ops.local_features, bit for bit).  candidates: ascending neighbourhood sizes; each
    point uses the one with the smallest eigenentropy."""
    rows, B, N = _cloud_rows(x)
    with torch.no_grad():
        idx = ops.knn_pm(rows, B, N, _list_length(k, candidates))
        out = ops.local_features(rows, idx, B, N, candidates=candidates, columns=columns)
    return out.view(B, N, -1)


def append_local_features(x, k=20, candidates=None, columns=DEFAULT_COLUMNS, zorder=False):
    """x [B,1,N,3] -> [B,1,N,3+len(columns)]: the coordinates with the selected columns behind them, written by ONE launch.
    zorder: reorder each cloud along a Z-order curve first (engine.reorder_points) -- the use_mFea trunks do not reorder their 8-column
    input themselves, and a Z-ordered cloud is what the kNN walk and the aggregation kernels are tuned for; the rows of the result then
    follow that order (PointNetVlad's descriptor does not depend on it)."""
    x = engine._check_input(x)
    with torch.no_grad():
        if zorder:
            x = engine.reorder_points(x)
        B, N = x.shape[0], x.shape[2]
        rows = x.view(B * N, 3)
        idx = ops.knn_pm(rows, B, N, _list_length(k, candidates))
        out = ops.local_features(rows, idx, B, N, candidates=candidates, columns=columns, copy_xyz=True)
    return out.view(B, 1, N, out.shape[1])


def _conv1_key(trunk):
    return "conv1_lpd.0.weight" if isinstance(trunk.conv1_lpd, nn.Sequential) else "conv1_lpd.weight"


def convert_to_local_features(model):
    """An xyz-only PointNetVlad with an `lpdnet` / `lpdnetorigin` trunk -> the same model with a use_mFea trunk (PointNetVlad itself
    never enables use_mFea, as in the reference): model.emb_nn is replaced by the same class built with use_mFea=True and the same
    t3d / tfea / use_relu / k / emb_dims; every tensor is copied, conv1's weight is widened from 3 to 8 input columns with the five new
    columns zero.  A checkpoint trained on xyz alone therefore gives the same descriptors until training moves the new columns.
    Parameter surgery only: works on CPU.  Returns `model`."""
    old = getattr(model, "emb_nn", None)
    from util.lpdnet_model import LPDNet, LPDNetOrign
    if not isinstance(old, (LPDNet, LPDNetOrign)):
        raise ValueError("convert_to_local_features: the model needs an 'lpdnet' or 'lpdnetorigin' trunk (model.emb_nn)")
    if old.use_mFea:
        return model
    new = type(old)(emb_dims=old.emb_dims, use_mFea=True, t3d=old.t3d, tfea=old.tfea, use_relu=old.use_relu, k=old.k)
    state = {name: t.detach().clone() for name, t in old.state_dict().items()}
    key = _conv1_key(old)
    w3 = state[key]
    w8 = w3.new_zeros((w3.shape[0], 8) + tuple(w3.shape[2:]))
    w8[:, :3] = w3
    state[key] = w8
    ref = next(old.parameters())
    new = new.to(device=ref.device, dtype=ref.dtype)
    new.load_state_dict(state, strict=True)
    new.train(old.training)
    for p_new, p_old in zip(new.parameters(), old.parameters()):
        p_new.requires_grad_(p_old.requires_grad)
    model.emb_nn = new
    return model


class LocalFeatureInput(nn.Module):
    """A use_mFea model behind the xyz-only interface: forward(x [B,1,N,3]) = module(append_local_features(x, ..., zorder=True)) on
    the current stream, in eval and in train mode; the features carry no gradient (they are functions of the input alone).  The
    wrapped model is `.module`, as with nn.DataParallel: harness.save_checkpoint / load_pretrained see the real model, and everything
    that takes an nn.Module (get_latent_vectors, update_vectors, evaluate_model, run_model, train_step, BatchPipeline, ingest) takes
    the wrapper unchanged."""

    def __init__(self, module, k=20, candidates=None, columns=DEFAULT_COLUMNS):
        super().__init__()
        self.module = module
        self.k = k
        self.candidates = tuple(candidates) if candidates else None
        self.columns = tuple(columns)

    def forward(self, x):
        return self.module(append_local_features(x, self.k, self.candidates, self.columns, zorder=True))
