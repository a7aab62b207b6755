"""Restatement of the Karras augmentation arithmetic (include/kdiff_hip.h, kd_augment_*; the reference's k_diffusion/augmentation.py:40-89) in
plain torch on the CPU, in whatever dtype the caller asks for: the fp64 evaluation is the reference of tests/test_augment_gpu.py, the fp32
evaluation of the same lines sets its tolerance.  Nothing here follows the kernel's decomposition: the matrices are chains of 3 x 3 products
of the factors as the formula lists them, the sampling point is M^-1 (c, r, 1) literally, and the taps are gathered by index.
"""
import json
import os

import numpy as np
import torch

from oracle import brownian as obrown

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.json")
A_SCALE = A_ANISO = 2 ** 0.2
A_TRANS = 1 / 8


def load_golden():
    return json.load(open(GOLDEN))


def _eye(B, dtype):
    return torch.eye(3, dtype=dtype).repeat(B, 1, 1)


def T(tx, ty):
    m = _eye(tx.shape[0], tx.dtype)
    m[:, 0, 2], m[:, 1, 2] = tx, ty
    return m


def S(sx, sy):
    m = _eye(sx.shape[0], sx.dtype)
    m[:, 0, 0], m[:, 1, 1] = sx, sy
    return m


def R(th):
    m = _eye(th.shape[0], th.dtype)
    m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1] = th.cos(), -th.sin(), th.sin(), th.cos()
    return m


def _chain(mats):
    out = mats[0]
    for m in mats[1:]:
        out = out @ m
    return out


def _consts(raw, H, W, a_scale, a_aniso, a_trans, dtype):
    a = raw.to(dtype)
    one = torch.ones(a.shape[0], dtype=dtype)
    s, n, t = (torch.tensor(v, dtype=dtype) for v in (a_scale, a_aniso, a_trans))
    return [a[:, i] for i in range(8)], one, s, n, t, one * (W / 2 - 0.5), one * (H / 2 - 0.5)


def forward_matrix(raw, H, W, a_scale=A_SCALE, a_aniso=A_ANISO, a_trans=A_TRANS, dtype=torch.float64):
    """M [B, 3, 3] acting on (x = column, y = row, 1), the factors in the reference's order."""
    (a0, a1, a2, a3, a4, a5, a6, a7), one, s, n, t, cx, cy = _consts(raw, H, W, a_scale, a_aniso, a_trans, dtype)
    return _chain([T(cx, cy), S(1 - 2 * a0, one), S(one, 1 - 2 * a1), S(s ** a2, s ** a2), R(-a3), R(a4), S(n ** a5, n ** -a5), R(-a4),
                   T(t * H * a6, t * W * a7), T(-cx, -cy)])


def inverse_matrix(raw, H, W, a_scale=A_SCALE, a_aniso=A_ANISO, a_trans=A_TRANS, dtype=torch.float64):
    """M^-1 [B, 3, 3]: the inverse factors in reverse order (no numeric inverse)."""
    (a0, a1, a2, a3, a4, a5, a6, a7), one, s, n, t, cx, cy = _consts(raw, H, W, a_scale, a_aniso, a_trans, dtype)
    return _chain([T(cx, cy), T(-t * H * a6, -t * W * a7), R(a4), S(n ** -a5, n ** a5), R(-a4), R(a3), S(s ** -a2, s ** -a2), S(one, 1 - 2 * a1),
                   S(1 - 2 * a0, one), T(-cx, -cy)])


def cond_of(raw, dtype=torch.float64):
    a = raw.to(dtype)
    a0, a1, a2, a3, a4, a5, a6, a7 = (a[:, i] for i in range(8))
    return torch.stack([a0, a1, a2, a3.cos() - 1, a3.sin(), a5 * a4.cos(), a5 * a4.sin(), a6, a7], dim=1)


def reflect(i, n):
    """numpy-pad 'reflect' index (d c b | a b c d | c b a) of integer tensor ``i`` on an axis of n samples: period 2 (n - 1), any distance."""
    period = 2 * (n - 1)
    j = torch.remainder(i, period)
    return torch.where(j > n - 1, period - j, j)


def cubic(t, p0, p1, p2, p3):
    return p1 + 0.5 * t * (p2 - p0 + t * (2 * p0 - 5 * p1 + 4 * p2 - p3 + t * (3 * (p1 - p2) + p3 - p0)))


def warp(x, minv):
    """y [B, C, H, W]: output pixel (c, r) = the Catmull-Rom interpolant of x[b] at M^-1 (c, r, 1), taps at floor - 1 .. + 2, reflect-folded.
    Runs in minv's dtype."""
    dtype = minv.dtype
    x = x.to(dtype)
    B, C, H, W = x.shape
    r, c = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    out = torch.empty_like(x)
    for b in range(B):
        m = minv[b]
        sx = m[0, 0] * c + m[0, 1] * r + m[0, 2]
        sy = m[1, 0] * c + m[1, 1] * r + m[1, 2]
        fx, fy = sx.floor(), sy.floor()
        tx, ty = sx - fx, sy - fy
        ix, iy = fx.long() - 1, fy.long() - 1
        lines = []
        for k in range(4):
            yy = reflect(iy + k, H)
            taps = [x[b][:, yy, reflect(ix + l, W)] for l in range(4)]
            lines.append(cubic(tx, *taps))
        out[b] = cubic(ty, *lines)
    return out


# ---- the draw: the counter contract of include/kdiff_hip.h restated in numpy (integer Philox exact; Box-Muller in float32 as oracle/brownian.py) ----

def draw(key, batch, a_prob):
    b = np.arange(batch, dtype=np.uint64)
    k = [obrown._philox(int(key) & (2 ** 64 - 1), b, (3 << 62) | j) for j in range(4)]
    u, rad, cos = obrown._unit24, obrown._radius, obrown._cos_rev
    p = np.float32(a_prob)

    def gate(w):
        return u(w) < p

    def angle(w):
        return ((u(w) - np.float32(0.5)) * np.float32(6.28318501)).astype(np.float32)

    def normal(wr, wa):
        return (rad(wr) * cos(u(wa))).astype(np.float32)
    zero = np.zeros(batch, dtype=np.float32)
    raw = np.zeros((batch, 8), dtype=np.float32)
    raw[:, 0] = (k[0][0] >> np.uint32(31)).astype(np.float32)
    raw[:, 1] = np.where(gate(k[0][1]), (k[0][2] >> np.uint32(31)).astype(np.float32), zero)
    raw[:, 2] = np.where(gate(k[0][3]), normal(k[1][0], k[1][1]), zero)
    raw[:, 3] = np.where(gate(k[1][2]), angle(k[1][3]), zero)
    g = gate(k[2][0])
    raw[:, 4] = np.where(g, angle(k[2][1]), zero)
    raw[:, 5] = np.where(g, normal(k[2][2], k[2][3]), zero)
    g = gate(k[3][0])
    r, rev = rad(k[3][2]), u(k[3][3])
    raw[:, 6] = np.where(g, r * cos(rev), zero)
    raw[:, 7] = np.where(g, r * cos(rev - np.float32(0.25)), zero)
    gates = np.stack([gate(k[0][1]), gate(k[0][3]), gate(k[1][2]), gate(k[2][0]), gate(k[3][0])], axis=1)
    return raw, gates
