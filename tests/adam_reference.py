"""fp64 reference of ONE Adam step (csrc/adam.hip, torch.optim.Adam) with per-element allowances, and the inputs the Adam
tests share (tests/test_adam_cpu.py, tests/test_gpu_adam.py).

torch on the CPU only; the HIP library is never loaded from here.

Every step is checked from the ACTUAL fp32 state in front of it - never against a free-running fp64 trajectory: with
sign-alternating gradients exp_avg cancels, and its relative distance to an fp64 trajectory reaches thousands of eps in any
correct fp32 Adam.  With g_eff = g + wd p (torch's coupled weight decay):
    m64 = b1 m + (1 - b1) g_eff
    v64 = b2 v + (1 - b2) g_eff^2
and the parameter against the update formed from the implementation's OWN rounded results m_out, v_out (the kernel forms
the update from these floats too):
    p64 = p - lr / (1 - b1^t) * m_out / (sqrt(v_out) / sqrt(1 - b2^t) + eps)                 all of it in fp64

Allowances: the roundings of adam_update (csrc/adam.hip; torch's fused_adam_utils.cuh is the same expressions) counted, with
a factor of two on top.  E = 2^-24 is the unit roundoff of fp32, 2^-149 its smallest denormal:
    m: |m_out - m64| <= 2^-23 (b1 |m| + (1 - b1)(|g| + wd |p|)) + 2^-149           one rounding of a sum formed in double
    v: |v_out - v64| <= 2^-21 (b2 v + (1 - b2)(|g| + wd |p|)^2) + 2^-149           g_eff is rounded once and then squared
    p: |p_out - p64| <= 2^-23 |p64| + 2^-20 |D| + 2^-149,   D = p - p64           seven roundings in D (step_size, sqrtf,
       the division by bc2_sqrt and its float argument, + eps, the product, the quotient), half an ulp in the final store
Where the fp64 formula is not finite (an inf or NaN gradient) the result must be non-finite in the same elements - and in
no other: `adam_ratios` returns inf for a tensor in which the two sets differ.
"""
import math
from collections import namedtuple

import torch

GRAD_SCALES = [1e-25, 1e-12, 1e-6, 1e-3, 1.0, 1e3, 1e9, 1e18]
TINY = 2.0 ** -149

AdamStep = namedtuple('AdamStep', 'm64 v64 p64 tol_m tol_v tol_p')


def _f64(x):
    return x.detach().to('cpu', torch.float64).reshape(-1)


def bias_corrections(t, betas):
    """(1 - b1^t, sqrt(1 - b2^t)) as 3dinfomax_amd/optim.py forms them; t: int or a tensor of per-element step counts"""
    b1, b2 = betas
    if torch.is_tensor(t):
        t = _f64(t)
        return 1 - torch.pow(torch.tensor(b1, dtype=torch.float64), t), torch.sqrt(1 - torch.pow(torch.tensor(b2, dtype=torch.float64), t))
    return 1 - b1 ** t, math.sqrt(1 - b2 ** t)


def adam_step_fp64(p, g, m, v, t, lr, betas, eps, weight_decay, m_out, v_out):
    """p, g, m, v: the fp32 tensors BEFORE the step; m_out, v_out: the implementation's exp_avg / exp_avg_sq AFTER it (they enter
    p64 only).  t: the step count of this step (1 for the first), an int or a per-element tensor.  Returns AdamStep, flat fp64."""
    p, g, m, v, m_out, v_out = (_f64(x) for x in (p, g, m, v, m_out, v_out))
    b1, b2 = betas
    g_eff = g + weight_decay * p
    m64 = b1 * m + (1 - b1) * g_eff
    v64 = b2 * v + (1 - b2) * g_eff * g_eff
    g_abs = g.abs() + weight_decay * p.abs()
    tol_m = 2.0 ** -23 * (b1 * m.abs() + (1 - b1) * g_abs) + TINY
    tol_v = 2.0 ** -21 * (b2 * v + (1 - b2) * g_abs * g_abs) + TINY
    bc1, bc2s = bias_corrections(t, betas)
    p64 = p - lr / bc1 * m_out / (torch.sqrt(v_out) / bc2s + eps)
    tol_p = 2.0 ** -23 * p64.abs() + 2.0 ** -20 * (p - p64).abs() + TINY
    return AdamStep(m64, v64, p64, tol_m, tol_v, tol_p)


def _ratio(out, ref, tol):
    out = _f64(out)
    fin = torch.isfinite(ref)
    if not torch.equal(torch.isfinite(out), fin):
        return math.inf                  # non-finite where the fp64 formula is finite, or the other way round
    inf = torch.isinf(ref)
    if bool(inf.any()) and not torch.equal(out[inf], ref[inf]):
        return math.inf                  # (an infinity of the other sign, or a NaN in its place)
    if not bool(fin.any()):
        return 0.0
    return float(((out[fin] - ref[fin]).abs() / tol[fin]).max())


def adam_ratios(p, g, m, v, p_out, m_out, v_out, t, lr, betas, eps, weight_decay):
    """largest error / allowance over the elements, for (exp_avg, exp_avg_sq, param); a value above 1 is outside the allowance"""
    r = adam_step_fp64(p, g, m, v, t, lr, betas, eps, weight_decay, m_out, v_out)
    return _ratio(m_out, r.m64, r.tol_m), _ratio(v_out, r.v64, r.tol_v), _ratio(p_out, r.p64, r.tol_p)


def unit(n, gen):
    """magnitudes in [0.5, 1.5): the squares of the largest gradient scale stay finite in fp32.  gen=None: exactly 1"""
    return torch.ones(n, dtype=torch.float64) if gen is None else torch.rand(n, generator=gen, dtype=torch.float64) + 0.5


def param_values(n, gen):
    """parameter scales 10^((i % 5) - 2); with a generator: random magnitudes around them, both signs"""
    i = torch.arange(n)
    sign = 1.0 if gen is None else 1.0 - 2.0 * torch.randint(0, 2, (n,), generator=gen).double()
    return (10.0 ** ((i % 5) - 2).double() * unit(n, gen) * sign).float()


def grad_values(n, gen, step=0, scale=None):
    """gradients of the scale list (element i: GRAD_SCALES[i % 8], or one `scale` for all), the sign alternating with the
    element AND with the step - exp_avg cancels from one step to the next"""
    i = torch.arange(n)
    s = torch.tensor(GRAD_SCALES, dtype=torch.float64)[i % len(GRAD_SCALES)] if scale is None else torch.full((n,), scale, dtype=torch.float64)
    sign = 1.0 - 2.0 * ((i + step) % 2).double()
    return (s * unit(n, gen) * sign).float()
