"""The feature-perturbation input of the decoder, `cat(x, Dropout2d(x[row0 : row0 + nu]))`, restated for the tests: the tensor-op
form in torch (the comparison of every GPU test, under autograd), a plain numpy loop over the elements (what the tensor-op form is
checked against on the host), and the masks the tests use."""
import numpy as np
import torch

SCALE = float(np.float32(1 / 0.7))  # a multiplier whose products round: fused and unfused multiply-adds differ in ~30 % of fp32 results


def tensor_ops(x: torch.Tensor, mask: torch.Tensor, row0: int) -> torch.Tensor:
    """x [N, H, W, C] (NHWC), mask fp32 [nu, C]: the definition of the issue, word for word."""
    nu = mask.shape[0]
    m = mask[:, None, None, :]
    return torch.cat((x, torch.where(m == 0, 0, x[row0:row0 + nu].float() * m).to(x.dtype)))


def tensor_ops_grad(x: torch.Tensor, mask: torch.Tensor, row0: int, dy: torch.Tensor):
    """(out, dx) of the tensor-op form under autograd."""
    leaf = x.detach().clone().requires_grad_(True)
    out = tensor_ops(leaf, mask, row0)
    out.backward(dy)
    return out.detach(), leaf.grad


def numpy_loop(x: np.ndarray, mask: np.ndarray, row0: int) -> np.ndarray:
    """fp32 x [N, H, W, C], fp32 mask [nu, C]: one element at a time."""
    n, h, w, c = x.shape
    nu = mask.shape[0]
    out = np.empty((n + nu, h, w, c), np.float32)
    for i in range(n):
        for p in range(h):
            for q in range(w):
                for ch in range(c):
                    out[i, p, q, ch] = x[i, p, q, ch]
    for u in range(nu):
        for p in range(h):
            for q in range(w):
                for ch in range(c):
                    m = np.float32(mask[u, ch])
                    out[n + u, p, q, ch] = np.float32(0.0) if m == 0 else np.float32(x[row0 + u, p, q, ch]) * m
    return out


def make_mask(nu: int, c: int, seed: int = 0) -> torch.Tensor:
    """fp32 [nu, c] of {0, 1 / 0.7}: row 1 all zero and row 2 all one (where there are that many rows: the arithmetic comes first);
    every other row random with at least one dropped and one kept channel (c >= 2)."""
    g = np.random.default_rng(seed)
    m = np.where(g.random((nu, c)) < 0.5, 0.0, SCALE).astype(np.float32)
    for u in range(nu):
        if u == 1:
            m[u] = 0.0
        elif u == 2:
            m[u] = 1.0
        elif c >= 2:
            a, b = g.choice(c, 2, replace=False)
            m[u, a], m[u, b] = 0.0, SCALE
    return torch.from_numpy(m)
