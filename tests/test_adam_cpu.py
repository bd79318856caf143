"""tests/adam_reference.py against torch.optim.Adam in fp32 on the CPU - no GPU, the HIP library is never loaded.

The allowances of adam_reference are aimed at csrc/adam.hip in tests/test_gpu_adam.py.  Here they are shown to hold for torch's
own fp32 Adam (both of its CPU implementations) with room to spare - and NOT to hold for a step that is subtly wrong: a bias
correction taken one step early, a dropped weight decay, swapped betas."""
import pytest
import torch

import adam_reference as R

N = 4097
STEPS = 8
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def _inputs():
    """one tensor per gradient scale: parameters exactly 10^((i % 5) - 2), gradients exactly +-scale with the sign alternating along
    the tensor and from step to step, eight steps.

    Exact scales and no random magnitudes, on purpose.  The exp_avg allowance counts the ONE rounding of csrc/adam.hip and of torch's
    fused kernel (the sum is formed in double).  torch's CPU Adam forms exp_avg as lerp(m, g, 1 - b1) in fp32 - three roundings of
    (1 - b1)(g - m) and one of the result - which is no larger than the allowance only while |m| is not small against |g|.  On these
    inputs it stays at 0.72 of it; with magnitudes drawn from [0.5, 1.5) around the same scales single elements reach 1.19 (measured,
    both foreach settings).  That is torch's CPU expression, not the kernel's: tests/test_gpu_adam.py aims the same allowances at the
    kernel WITH random magnitudes, and `test_the_allowances_reject_a_wrong_step` below holds the kernel's expression order to 0.5 on them."""
    params = [R.param_values(N, None) for _ in R.GRAD_SCALES]
    grads = [[R.grad_values(N, None, step=s, scale=sc) for sc in R.GRAD_SCALES] for s in range(STEPS)]
    return params, grads


@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('foreach', [False, True])
def test_torch_fp32_adam_is_inside_the_allowances(foreach, wd):
    params, grads = _inputs()
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=foreach)
    worst = [0.0, 0.0, 0.0]
    for s in range(STEPS):
        pre = []
        for p, g in zip(ps, grads[s]):
            p.grad = g.clone()
            st = opt.state[p]
            pre.append((p.detach().clone(), g, st['exp_avg'].clone() if st else torch.zeros(N), st['exp_avg_sq'].clone() if st else torch.zeros(N)))
        opt.step()
        for k, (p, (p0, g, m0, v0)) in enumerate(zip(ps, pre)):
            st = opt.state[p]
            assert float(st['step']) == s + 1
            ratios = R.adam_ratios(p0, g, m0, v0, p.detach(), st['exp_avg'], st['exp_avg_sq'], s + 1, LR, BETAS, EPS, wd)
            assert max(ratios) <= 1.0, (s + 1, R.GRAD_SCALES[k], ratios)
            worst = [max(a, b) for a, b in zip(worst, ratios)]
    print(f'torch fp32 CPU Adam foreach={foreach} wd={wd}: worst error / allowance  m {worst[0]:.3f}  v {worst[1]:.3f}  p {worst[2]:.3f}')
    # room to spare: a helper whose allowances were loosened further would show here as ratios that shrink, one whose formula drifted
    # from torch's as ratios that grow
    assert max(worst) < 0.8, worst


def _step_f32(p, g, m, v, t, lr, betas, eps, wd):
    """one Adam step in fp64 from fp32 inputs, every result rounded to fp32 once: the most accurate fp32 step there is"""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    g = g + wd * p
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    m32, v32 = m.float(), v.float()
    bc1, bc2s = R.bias_corrections(t, betas)
    p = p - lr / bc1 * m32.double() / (v32.double().sqrt() / bc2s + eps)
    return p.float(), m32, v32


WRONG = {
    'bias corrections of step t - 1': lambda p, g, m, v, t, wd: _step_f32(p, g, m, v, t - 1, LR, BETAS, EPS, wd),
    'weight decay dropped': lambda p, g, m, v, t, wd: _step_f32(p, g, m, v, t, LR, BETAS, EPS, 0.0),
    'betas swapped': lambda p, g, m, v, t, wd: _step_f32(p, g, m, v, t, LR, BETAS[::-1], EPS, wd),
}


@pytest.mark.parametrize('t', [2, 3, 4])
def test_the_allowances_reject_a_wrong_step(t):
    wd = 1e-2
    gen = torch.Generator().manual_seed(99 + t)
    p, m, v = R.param_values(N, gen), torch.zeros(N), torch.zeros(N)
    for s in range(1, t):                                    # the true fp32 state in front of step t
        p, m, v = _step_f32(p, R.grad_values(N, gen, step=s), m, v, s, LR, BETAS, EPS, wd)
    g = R.grad_values(N, gen, step=t)
    right = R.adam_ratios(p, g, m, v, *_step_f32(p, g, m, v, t, LR, BETAS, EPS, wd), t, LR, BETAS, EPS, wd)
    print(f't={t} correct step: ratios {right}')
    assert max(right) <= 0.5 + 1e-6, right                   # one rounding each where the allowance counts two and more
    for name, fn in WRONG.items():
        r = R.adam_ratios(p, g, m, v, *fn(p, g, m, v, t, wd), t, LR, BETAS, EPS, wd)
        print(f't={t} {name}: ratios {r}')
        assert max(r) > 100, (name, r)
    # which quantity catches what: the early bias correction moves the parameter alone; the other two are in exp_avg / exp_avg_sq
    early = R.adam_ratios(p, g, m, v, *WRONG['bias corrections of step t - 1'](p, g, m, v, t, wd), t, LR, BETAS, EPS, wd)
    assert early[0] <= 1 and early[1] <= 1 and early[2] > 100, early
