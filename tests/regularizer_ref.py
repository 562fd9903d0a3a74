"""numpy fp64 restatement of the surface regularisers (artist/optim/regularizers.py:60-186) and of their autograd, for the tests
of artist_amd.regularizers.  The adjoint of the clamped Laplacian is written as what autograd does - a scatter of the four shifted
slices into the padded net, then the replicate pad's backward folding the border onto the edge - not as the stencil itself, so
that the kernel's use of the stencil as its own adjoint is checked, not assumed."""
import numpy as np

REDUCTIONS = [(1,), (0,), (0, 1)]


def laplacian(d):
    """The reference's Laplacian of d [H,F,U,V,3] with replicate padding."""
    p = np.pad(d, ((0, 0), (0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    return (((4 * d - p[:, :, :-2, 1:-1]) - p[:, :, 2:, 1:-1]) - p[:, :, 1:-1, :-2]) - p[:, :, 1:-1, 2:]


def laplacian_adjoint(x):
    """L^T x for x [H,F,U,V,3]: the autograd of `laplacian`."""
    H, F, U, V, C = x.shape
    gp = np.zeros((H, F, U + 2, V + 2, C))
    gp[:, :, :-2, 1:-1] -= x
    gp[:, :, 2:, 1:-1] -= x
    gp[:, :, 1:-1, :-2] -= x
    gp[:, :, 1:-1, 2:] -= x
    # replicate pad backward: the padded rows / columns belong to the edge row / column they copy
    gp[:, :, 1] += gp[:, :, 0]
    gp[:, :, -2] += gp[:, :, -1]
    gp[:, :, :, 1] += gp[:, :, :, 0]
    gp[:, :, :, -2] += gp[:, :, :, -1]
    return 4 * x + gp[:, :, 1:-1, 1:-1]


def terms(current, original):
    """(smoothness [H,F], ideal [H,F]) before the reduction."""
    d = np.asarray(current, np.float64) - np.asarray(original, np.float64)
    return (laplacian(d) ** 2).mean(axis=(2, 3, 4)), (d ** 2).mean(axis=(2, 3, 4))


def upstream(weights, reduction, shape_hf):
    """d(sum(weights * per_net.sum(reduction))) / d per_net, as [H,F]."""
    w = np.asarray(weights, np.float64)
    if reduction == (1,):
        w = w[:, None]
    elif reduction == (0,):
        w = w[None, :]
    return np.broadcast_to(w, shape_hf)


def gradients(current, original, grad_smoothness, grad_ideal):
    """Gradient w.r.t. current of sum(grad_smoothness * S) and of sum(grad_ideal * I), both [H,F] upstream."""
    d = np.asarray(current, np.float64) - np.asarray(original, np.float64)
    n = d.shape[2] * d.shape[3] * d.shape[4]
    gs = np.asarray(grad_smoothness, np.float64)[:, :, None, None, None]
    gi = np.asarray(grad_ideal, np.float64)[:, :, None, None, None]
    return gs * (2.0 / n) * laplacian_adjoint(laplacian(d)), gi * 2.0 * d / n


def reduce(per_net, reduction):
    return per_net.sum(axis=reduction)
