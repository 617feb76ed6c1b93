"""Torch reference of the Winograd F(2,3) form of a dilated Conv1d (hipops.ALGO_WINO, csrc/v2w_wino.h): the weight transform, the
fragment order of its packed stream, and the convolution computed through it.  Shared by tests/test_wino_cpu.py and tests/test_wino_gpu.py."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def segments(k):
    """(first tap, tap count) of each segment: k = 3 -> 3, 7 -> 3+3+1, 11 -> 3+3+3+2."""
    out, s0 = [], 0
    while s0 < k:
        n = min(3, k - s0)
        out.append((s0, n))
        s0 += n
    return out


# accumulator class of each term of a 3- / 2- / 1-tap segment
CLASSES = {3: (0, 1, 2, 3), 2: (0, 1, 3), 1: (0, 3)}


def transform(n, g):
    """Transformed weights of one segment from its taps g[0..n) (same fp32 arithmetic as the packers)."""
    if n == 3:
        g0, g1, g2 = g
        return [g0, ((g0 + g2) + g1) * 0.5, ((g0 + g2) - g1) * 0.5, g2]
    if n == 2:
        return [g[0], g[0] + g[1], g[1]]
    return [g[0], -g[0]]


def terms(k):
    return sum(len(CLASSES[n]) for _s0, n in segments(k))


def pack_ref(wf):
    """wf [k][C_in][C_out] -> the v2w_pack_wino stream: [32-row block][32-channel chunk][segment][unit gg][term][lane][j], where fragment
    (segment, gg, term) holds G[ch*32 + gg*8 + 2j + lane//32][mb*32 + lane%32]."""
    k, ci, co = wf.shape
    frags = []
    for s0, n in segments(k):
        gs = transform(n, [wf[s0 + j] for j in range(n)])
        for gg in range(4):
            frags += [(G, gg) for G in gs]
    lane = torch.arange(64)
    j = torch.arange(4)
    out = torch.empty((co // 32, ci // 32, len(frags), 64, 4), dtype=wf.dtype)
    for fi, (G, gg) in enumerate(frags):
        c_off = gg * 8 + 2 * j[None, :] + (lane // 32)[:, None]          # (64, 4)
        col = (lane % 32)[:, None].expand(64, 4)
        Gr = G.reshape(ci // 32, 32, co // 32, 32)
        out[:, :, fi] = Gr[:, c_off, :, col].permute(3, 2, 0, 1)         # (64, 4, nch, nmb) -> (nmb, nch, 64, 4)
    return out.reshape(-1)


def pack_ref_loop(wf):
    """pack_ref spelled out element by element (small shapes only): the layout's definition."""
    k, ci, co = wf.shape
    out = []
    for mb in range(co // 32):
        for ch in range(ci // 32):
            for s0, n in segments(k):
                for gg in range(4):
                    for t in range(len(CLASSES[n])):
                        for lane in range(64):
                            for j in range(4):
                                c, o = ch * 32 + gg * 8 + 2 * j + lane // 32, mb * 32 + lane % 32
                                out.append(transform(n, [wf[s0 + q, c, o] for q in range(n)])[t])
    return torch.stack(out)


def conv1d(x, w, bias, dilation=1, padding=None):
    """F.conv1d(x, w, bias, padding=dil*(k-1)//2, dilation=dil) (odd k, stride 1) through the four accumulator classes of output pairs
    (t, t + dil): M_c += G_c u_c per segment, y(t) = M0 + M1 + M2, y(t + dil) = M1 - M2 - M3."""
    B, ci, L = x.shape
    co, _, k = w.shape
    d = dilation
    hl = d * (k - 1) // 2
    assert padding is None or padding == hl
    npairs = d * ((L + 2 * d - 1) // (2 * d))
    P = torch.arange(npairs)
    t = 2 * d * (P // d) + P % d
    xp = F.pad(x, (hl, hl + 4 * d))                       # index t + (s0 + j) d of xp is position t - hl + (s0 + j) d
    wf = w.permute(2, 1, 0)                               # [k][C_in][C_out]
    M = [torch.zeros((B, co, npairs), dtype=x.dtype) for _ in range(4)]
    for s0, n in segments(k):
        xs = [xp[:, :, t + (s0 + j) * d] for j in range(n + 1)]
        if n == 3:
            us = [xs[0] - xs[2], xs[1] + xs[2], xs[2] - xs[1], xs[1] - xs[3]]
        elif n == 2:
            us = [xs[0] - xs[1], xs[1], xs[1] - xs[2]]
        else:
            us = [xs[0], xs[1]]
        for cls, G, u in zip(CLASSES[n], transform(n, [wf[s0 + q] for q in range(n)]), us):
            M[cls] = M[cls] + torch.einsum('io,bip->bop', G, u)
    y = torch.zeros((B, co, L + 4 * d), dtype=x.dtype)
    y[:, :, t] = (M[0] + M[1]) + M[2]
    y[:, :, t + d] = (M[1] - M[2]) - M[3]
    y = y[:, :, :L]
    return y if bias is None else y + bias[None, :, None]
