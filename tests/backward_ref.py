"""fp64 CPU references of the generator's parameter-space backward operations, and the forward-error bounds their GPU tests use.

Every reference is torch autograd through the DEFINITION of the operation (oracle/vec2wav_oracle.py spells the forward out), never
through the closed forms the kernels of csrc/v2w_backward.hip evaluate.  tests/test_backward_ref_cpu.py pins them against central
finite differences and against the whole-model oracle gradients.

The bounds are functions of the reference's own data (u = 2^-24 is the fp32 unit roundoff); none of them was read off a kernel.
"""
from types import SimpleNamespace

import torch

from oracle import vec2wav_oracle as O

U = 2.0 ** -24           # fp32 unit roundoff
CHAIN = 128              # allowance for the length of an fp32 partial chain before it is folded into fp64


def _f64(t):
    return None if t is None else t.detach().to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------
# references
def cbn_ref(dx, xr, gb, training, running_mean, running_var, eps=O.BN_EPS):
    """Conditional BatchNorm  x = gamma[b,c] * BN(xr) + beta[b,c],  gb = [gamma | beta] (B, 2C): (dxr, dgb) for the cotangent dx."""
    assert eps == O.BN_EPS, 'the oracle batch norm has a fixed eps'
    xr = _f64(xr).requires_grad_(True)
    gb = _f64(gb).requires_grad_(True)
    xhat, _, _ = O.batch_norm_no_affine(xr, _f64(running_mean), _f64(running_var), training)
    gamma, beta = gb.chunk(2, 1)
    x = gamma[:, :, None] * xhat + beta[:, :, None]
    dxr, dgb = torch.autograd.grad(x, (xr, gb), _f64(dx))
    return dxr, dgb


def cbn_centered_moment(dxr, xr):
    """sum_{b,l} dxr * (xr - mean) per channel, in fp64."""
    dxr, xr = _f64(dxr), _f64(xr)
    return (dxr * (xr - xr.mean(dim=(0, 2), keepdim=True))).sum(dim=(0, 2))


def cbn_centered_moment_ref(dx, xr, gb, eps=O.BN_EPS):
    """What `cbn_centered_moment` of the train-mode dxr is in exact arithmetic.  With xhat = (xr - mean) rstd, rstd = (var + eps)^-1/2:
    dxr = rstd (gamma dx - mean(gamma dx) - xhat mean(gamma dx xhat)) and mean(xhat^2) = var / (var + eps), so

        sum dxr = 0   and   sum dxr (xr - mean) = eps rstd^3 sum gamma dx (xr - mean)

    - the second moment vanishes only for eps = 0; what is left of it is this small multiple of the gamma-weighted input moment."""
    dx, xr, gb = _f64(dx), _f64(xr), _f64(gb)
    C = dx.shape[1]
    xc = xr - xr.mean(dim=(0, 2), keepdim=True)
    var = xr.var(dim=(0, 2), unbiased=False)
    return eps * (var + eps) ** -1.5 * (gb[:, :C, None] * dx * xc).sum(dim=(0, 2))


def cond_ref(dgb, W, b, u, v, fc_w, fc_b, spk, noise):
    """One stage's conditioning  z = fc_w cat(spk, noise) + fc_b,  sigma = u^T W v (u, v constants),  gb = (W / sigma) z + b:
    (d W, d b, d fc_w, d fc_b) for the cotangent dgb."""
    W, b, fc_w, fc_b = (_f64(t).requires_grad_(True) for t in (W, b, fc_w, fc_b))
    u, v = _f64(u), _f64(v)
    sn = torch.cat((_f64(spk), _f64(noise)), dim=1)
    z = sn @ fc_w.t() + fc_b
    sigma = torch.dot(u, torch.mv(W, v))
    gb = z @ (W / sigma).t() + b
    return torch.autograd.grad(gb, (W, b, fc_w, fc_b), _f64(dgb))


def wf_to_param_layout(dwf, transposed):
    """[k][C_in][C_out] -> the parameter's layout: (C_in, C_out, k) of a ConvTranspose1d, (C_out, C_in, k) of a Conv1d."""
    return (dwf.permute(1, 2, 0) if transposed else dwf.permute(2, 1, 0)).contiguous()


def param_to_wf_layout(w, transposed):
    """The inverse of `wf_to_param_layout`."""
    return (w.permute(2, 0, 1) if transposed else w.permute(2, 1, 0)).contiguous()


def wn_ref(dwf, v, g, transposed):
    """Weight norm  w = g * v / ||v||  (norm over all dimensions but 0), cotangent dwf in the [k][C_in][C_out] layout: (dv, dg);
    with g None the parameter is the weight itself and dv is the relayout of dwf (dg None)."""
    if g is None:
        return wf_to_param_layout(dwf, transposed), None
    dw = wf_to_param_layout(_f64(dwf), transposed)
    v = _f64(v).requires_grad_(True)
    g = _f64(g).requires_grad_(True)
    norm = v.pow(2).sum(dim=tuple(range(1, v.dim())), keepdim=True).sqrt()
    w = g * v / norm
    dv, dg = torch.autograd.grad(w, (v, g), dw)
    return dv, dg


# ---------------------------------------------------------------------------------------------------------------
# forward-error bounds (all arguments fp64 reference data)
def sum_bound(abs_sum, total):
    """|err| of a sum of terms t_i done with fp32 partial chains: 128 u sum|t_i| + 2 u |sum t_i|."""
    return CHAIN * U * abs_sum + 2 * U * total.abs()


def cbn_bounds(dx, xr, gb, training, running_mean, running_var, eps=O.BN_EPS):
    """Bounds for `cbn_backward` against `cbn_ref`: a namespace with `dxr` (per element), `dgb` (per entry) and `terms`, the summed
    magnitudes |a dx| + |bc xr| + |cc| of the three products every element of dxr is made of (for the train-mode identities).

      S1 = sum_l dx, S2 = sum_l dx*xr per (b, c):     sum_bound each
      dbeta = S1, dgamma = rstd*(S2 - mean*S1):       rstd*(bound(S2) + |mean|*bound(S1))  - grows with |mean|/std of the channel
      dxr = a*dx + bc*xr + cc  elementwise in fp32:   4u(|a dx| + |bc xr| + |cc|)  plus the propagated bounds of bc and cc, which are
        bc = -rstd^2 m2,  cc = -rstd m1 + rstd^2 mean m2,  m1 = sum_b gamma dbeta / n,  m2 = sum_b gamma dgamma / n  (n = B L):
        bound(m1) = sum_b |gamma| bound(S1) / n,  bound(m2) = sum_b |gamma| bound(dgamma) / n.
      The single roundings to fp32 on the way (S1, S2, dgb; a, bc, cc and the two fused multiply-adds) are inside the 2u and 4u factors.
    """
    dx, xr, gb = _f64(dx), _f64(xr), _f64(gb)
    B, C, L = dx.shape
    n = B * L
    gamma = gb[:, :C]
    if training:
        mean = xr.mean(dim=(0, 2))
        var = xr.var(dim=(0, 2), unbiased=False)
    else:
        mean, var = _f64(running_mean), _f64(running_var)
    rstd = torch.rsqrt(var + eps)
    S1, S2 = dx.sum(2), (dx * xr).sum(2)
    bS1 = sum_bound(dx.abs().sum(2), S1)
    bS2 = sum_bound((dx * xr).abs().sum(2), S2)
    dgamma = rstd * (S2 - mean * S1)
    b_dgamma = rstd * (bS2 + mean.abs() * bS1)
    b_dgb = torch.cat((b_dgamma, bS1), dim=1)
    a = gamma * rstd                                                         # (B, C)
    if training:
        m1 = (gamma * S1).sum(0) / n
        m2 = (gamma * dgamma).sum(0) / n
        b_m1 = (gamma.abs() * bS1).sum(0) / n
        b_m2 = (gamma.abs() * b_dgamma).sum(0) / n
        bc = -rstd * rstd * m2
        cc = -rstd * m1 + rstd * rstd * mean * m2
        b_bc = rstd * rstd * b_m2
        b_cc = rstd * b_m1 + rstd * rstd * mean.abs() * b_m2
    else:
        bc = cc = b_bc = b_cc = torch.zeros(C, dtype=torch.float64)
    terms = (a[:, :, None] * dx).abs() + (bc[None, :, None] * xr).abs() + cc.abs()[None, :, None]
    b_dxr = 4 * U * terms + b_bc[None, :, None] * xr.abs() + b_cc[None, :, None]
    return SimpleNamespace(dxr=b_dxr, dgb=b_dgb, terms=terms)


def cond_bounds(dgb, W, b, u, v, fc_w, fc_b, spk, noise, sigma_used):
    """Bounds on (d W, d b, d fc_w, d fc_b) of `cond_backward` against `cond_ref`.  Every sum over n terms in fp32 costs
    (n + 2) u sum|t_i|; a value built from such sums carries their bounds through its formula:

      dWhat[r,j] = sum_b dgb[b,r] z[b,j]                     n = B
      tot        = sum_{r,j} dWhat[r,j] W[r,j]               n = 128 R, plus sum |W| bound(dWhat)
      dW         = dWhat/sigma - tot/sigma^2 u[r] v[j]       one u per fp32 operation: 4u on the first term, 6u on the second
      dz[b,j]    = sum_r dgb[b,r] W[r,j] / sigma             n = R
      dfc_w[j,i] = sum_b dz[b,j] sn[b,i]                     n = B, plus sum_b |sn| bound(dz)

    `sigma_used` is the fp32 value of u^T W v handed to the kernel (the forward computes it in fp32).  It differs from the fp64 sigma
    by dsig - a perturbation of an INPUT, known exactly here - which moves 1/sigma by dsig/sigma^2 and 1/sigma^2 by 2 dsig/sigma^3."""
    dgb, W, u, v = _f64(dgb), _f64(W), _f64(u), _f64(v)
    sn = torch.cat((_f64(spk), _f64(noise)), dim=1)
    B, R = dgb.shape
    z = sn @ _f64(fc_w).t() + _f64(fc_b)
    sigma = torch.dot(u, torch.mv(W, v))
    rs = abs(float(sigma_used) - sigma.item()) / abs(sigma.item()) + U      # relative error of the 1/sigma the kernel uses
    s = sigma.abs()
    dWhat = dgb.t() @ z
    a_dWhat = dgb.abs().t() @ z.abs()
    b_dWhat = (B + 2) * U * a_dWhat + U * a_dWhat                             # + z handed over rounded to fp32
    tot = (dWhat * W).sum()
    b_tot = (128 * R + 2) * U * (dWhat * W).abs().sum() + (W.abs() * b_dWhat).sum()
    uv = torch.outer(u, v).abs()
    b_dW = (b_dWhat / s + b_tot / s ** 2 * uv
            + (4 * U + rs) * dWhat.abs() / s + (6 * U + 2 * rs) * tot.abs() / s ** 2 * uv)
    b_db = (B + 2) * U * dgb.abs().sum(0)
    dz = dgb @ W / sigma
    a_dz = dgb.abs() @ W.abs() / s
    b_dz = (R + 2) * U * a_dz + (2 * U + rs) * dz.abs()
    b_dfw = (B + 2) * U * (dz.abs().t() @ sn.abs()) + b_dz.t() @ sn.abs()
    b_dfb = (B + 2) * U * dz.abs().sum(0) + b_dz.sum(0)
    return b_dW, b_db, b_dfw, b_dfb


def wn_bounds(dwf, v, g, transposed):
    """Bounds on (dv, dg) of `wn_backward` (fp64 inside, rounded once): 4u(|dw| + |v| |<dw,v>| / ||v||^2) |g| / ||v|| per element of dv,
    2u |dg| per row."""
    dw = wf_to_param_layout(_f64(dwf), transposed)
    v, g = _f64(v), _f64(g)
    dims = tuple(range(1, v.dim()))
    n2 = v.pow(2).sum(dim=dims, keepdim=True)
    norm = n2.sqrt()
    dot = (dw * v).sum(dim=dims, keepdim=True)
    b_dv = 4 * U * (dw.abs() + v.abs() * dot.abs() / n2) * g.abs() / norm
    b_dg = 2 * U * (dot / norm).abs()
    return b_dv, b_dg


def worst_ratio(got, want, bound):
    """max over entries of |got - want| / bound (0/0 counts as 0, x/0 as inf): <= 1 means the bound holds everywhere."""
    err = (_f64(got) - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isfinite(_f64(got)), ratio, torch.full_like(ratio, float('inf')))
    return ratio.max().item() if ratio.numel() else 0.0
