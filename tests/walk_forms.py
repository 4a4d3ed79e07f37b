"""The layouts of one (cloud, lists) input that take the other read paths of the list walk (csrc/lpd_list_walk.h), for
lpd_local_features and lpd_point_normals alike.  A plain input -- coordinates [B*N, 3] and lists [B, N, K], both contiguous on a
16-byte aligned base -- stages a contiguous cloud in 16-byte pieces and, with K % 4 == 0, reads a list as int4 pieces; each form
below holds the same values and must give the same bits."""
import torch


def off_alignment(t):
    """the values of t at a base 4 bytes past a 16-byte boundary: a view from element 1 of a buffer one element longer"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def forms(rows, idx):
    """rows [B*N, 3] fp32, idx [B, N, K] int32 on the device, plain -> [(name, rows, idx)]: the lists off alignment (4-byte loads
    whatever K), the coordinates as the first three columns of a [B*N, 4] tensor (ldx = 4: staged by the float; the fourth column is
    NaN and never read) and as [B*N, 3] off alignment (ldx = 3, staged by the float)"""
    assert rows.is_contiguous() and idx.is_contiguous() and rows.data_ptr() % 16 == 0 and idx.data_ptr() % 16 == 0
    wide = torch.full((rows.shape[0], 4), float("nan"), dtype=rows.dtype, device=rows.device)
    wide[:, :3] = rows
    return [("lists+4", rows, off_alignment(idx)), ("ldx=4", wide[:, :3], idx), ("xyz+4", off_alignment(rows), idx)]
