"""Plain float64 reference of ConvTranspose3d(kernel 2, stride 2, bias) and its gradients (test infrastructure).

With kernel == stride every fine voxel receives exactly one tap, so the op is one GEMM and a scatter:
    Y[v, (co, i, j, l)] = A[v, :] @ W[:, (co, i, j, l)]          A: [V x Ci] coarse voxels, W: [Ci x 8 Co] (torch layout)
    out[n, co, 2d + i, 2h + j, 2w + l] = Y[(n, d, h, w), (co, i, j, l)] + b[co]
and the gradients are the two other GEMMs of the same three matrices.  One BLAS matmul keeps a 128 -> 128 case at 16 k
voxels well under a second on the host, where F.conv_transpose3d in float64 takes many.  tests/test_convt_ref_cpu.py holds
these functions to F.conv_transpose3d with autograd."""
import torch


def activate(x, scale=None, shift=None, relu=True, store=None):
    """relu(x * scale + shift) per channel of an NCDHW tensor, in float64 (the transform a consumer applies to its lazily
    normalised input); None = identity.  store: the 16-bit type the kernel rounds the transformed value to before it
    multiplies (float64 -> float32 -> store, the roundings of a float32 fma followed by the conversion)."""
    a = x.double()
    if scale is not None:
        c = x.shape[1]
        a = a * scale[:c].double().view(1, -1, 1, 1, 1) + shift[:c].double().view(1, -1, 1, 1, 1)
        if relu:
            a = a.clamp_min(0.0)
        if store is not None:
            a = a.float().to(store).double()
    return a


def _rows(a):
    """NCDHW -> [V x C], V = (n, d, h, w) with w fastest."""
    return a.double().permute(0, 2, 3, 4, 1).reshape(-1, a.shape[1])


def _gather(g, co):
    """Fine NCDHW gradient / output [N, Co, 2D, 2H, 2W] -> [V x (co, i, j, l)] over the coarse voxels."""
    n, _, d2, h2, w2 = g.shape
    t = g.double().view(n, co, d2 // 2, 2, h2 // 2, 2, w2 // 2, 2)
    return t.permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(-1, co * 8)


def forward(a, w, b=None):
    """a [N, Ci, D, H, W] (already activated), w [Ci, Co, 2, 2, 2], b [Co] -> float64 [N, Co, 2D, 2H, 2W]."""
    n, ci, d, h, wd = a.shape
    co = w.shape[1]
    y = _rows(a) @ w.double().reshape(ci, co * 8)
    y = y.view(n, d, h, wd, co, 2, 2, 2).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(n, co, 2 * d, 2 * h, 2 * wd)
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1, 1)
    return y


def data_gradient(g, w):
    """g [N, Co, 2D, 2H, 2W], w [Ci, Co, 2, 2, 2] -> gradient of the (activated) input, float64 [N, Ci, D, H, W]."""
    n, co, d2, h2, w2 = g.shape
    ci = w.shape[0]
    dx = _gather(g, co) @ w.double().reshape(ci, co * 8).t()
    return dx.view(n, d2 // 2, h2 // 2, w2 // 2, ci).permute(0, 4, 1, 2, 3).contiguous()


def weight_gradient(a, g):
    """a [N, Ci, D, H, W] (already activated), g [N, Co, 2D, 2H, 2W] -> (dw [Ci, Co, 2, 2, 2], db [Co]) in float64."""
    ci, co = a.shape[1], g.shape[1]
    dw = _rows(a).t() @ _gather(g, co)
    return dw.view(ci, co, 2, 2, 2), g.double().sum((0, 2, 3, 4))
