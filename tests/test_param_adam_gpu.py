"""optim.ParamAdam on the GPU: its steps are the tg_counter_inc / tg_adam_step launches a caller would issue by hand, and a parameter without a
gradient is skipped whole (value and moments untouched) while the counter advances.  Both sides run the same kernel: bit equality, no
tolerance."""
import pytest
import torch

SIZES = (8, 5, 12)                  # 5: not a multiple of four
LR, BETAS, EPS = 1e-3, (0.5, 0.999), 1e-8


@pytest.mark.gpu
def test_param_adam_steps_live_parameters_and_skips_the_rest_bit_for_bit(pkg, dev):
    ops = pkg.ops
    gen = torch.Generator().manual_seed(7)
    draw = lambda n: torch.randn(n, generator=gen).to(dev)
    init = [draw(n) for n in SIZES]
    params = [torch.nn.Parameter(t.clone()) for t in init]
    adam = pkg.ParamAdam(params, LR, BETAS, EPS)
    # the same steps by hand on clones
    ref_p = [t.clone() for t in init]
    ref_m, ref_v = [torch.zeros_like(t) for t in init], [torch.zeros_like(t) for t in init]
    ref_step = torch.zeros(1, device=dev, dtype=torch.int32)
    for _ in range(3):
        grads = [draw(n) for n in SIZES]
        adam.zero_grad()
        assert all(p.grad is None for p in params)
        params[0].grad, params[2].grad = grads[0].clone(), grads[2].clone()
        assert [g.data_ptr() for g in adam.live_grads()] == [params[0].grad.data_ptr(), params[2].grad.data_ptr()]
        adam.step()
        ops.counter_inc(ref_step)
        for i in (0, 2):
            ops.adam_step(ref_p[i], grads[i], ref_m[i], ref_v[i], LR, BETAS[0], BETAS[1], EPS, ref_step)
    assert int(adam.step_dev) == 3
    for i in (0, 2):
        assert torch.equal(params[i].data, ref_p[i]) and torch.equal(adam.m[i], ref_m[i]) and torch.equal(adam.v[i], ref_v[i]), i
        assert not torch.equal(params[i].data, init[i])
    assert torch.equal(params[1].data, init[1]) and not adam.m[1].any() and not adam.v[1].any()
    # the skipped parameter's first own step is step 4 of the optimiser: the bias corrections of a counter holding 4
    g1 = draw(SIZES[1])
    adam.zero_grad()
    params[1].grad = g1.clone()
    adam.step()
    four = torch.full((1,), 4, device=dev, dtype=torch.int32)
    ops.adam_step(ref_p[1], g1, ref_m[1], ref_v[1], LR, BETAS[0], BETAS[1], EPS, four)
    assert int(adam.step_dev) == 4
    assert torch.equal(params[1].data, ref_p[1]) and torch.equal(adam.m[1], ref_m[1]) and torch.equal(adam.v[1], ref_v[1])
    assert not torch.equal(params[1].data, init[1])
    for i in (0, 2):                # and this step left the two others alone
        assert torch.equal(params[i].data, ref_p[i]) and torch.equal(adam.m[i], ref_m[i]) and torch.equal(adam.v[i], ref_v[i]), i


@pytest.mark.gpu
def test_live_grads_makes_a_strided_gradient_contiguous_in_place(pkg, dev):
    p = torch.nn.Parameter(torch.zeros(4, 3, device=dev))
    adam = pkg.ParamAdam([p], LR, BETAS, EPS)
    p.grad = torch.arange(12.0, device=dev).view(3, 4).t()
    (g,) = adam.live_grads()
    assert g is p.grad and g.is_contiguous() and torch.equal(g, torch.arange(12.0, device=dev).view(3, 4).t())
