"""CPU-side checks of optim.adopt: the three baseline train_iter_* functions refuse, before a tensor is touched, every torch optimiser whose
settings the device Adam (optim.ParamAdam) cannot honour, and keep one trainer per optimiser and network.  No GPU needed."""
from types import SimpleNamespace

import pytest
import torch

MESSAGE = " steps with the device Adam: pass a torch.optim.Adam with one parameter group, no weight_decay, no amsgrad"
ARGS = SimpleNamespace(loss_regression_weight=100.0, loss_gan_weight=10.0, loss_kld_weight=0.1, loss_reg_weight=0.1, n_pre_poses=4)


def good(mod):
    return torch.optim.Adam(mod.parameters(), lr=1e-3, betas=(0.5, 0.999))


BAD = {
    "sgd": lambda mod: torch.optim.SGD(mod.parameters(), lr=1e-3),
    "two_groups": lambda mod: torch.optim.Adam([{"params": [mod.weight]}, {"params": [mod.bias]}], lr=1e-3),
    "weight_decay": lambda mod: torch.optim.Adam(mod.parameters(), lr=1e-3, weight_decay=1e-2),
    "amsgrad": lambda mod: torch.optim.Adam(mod.parameters(), lr=1e-3, amsgrad=True),
}


def run(pkg, which, bad):
    """Calls one train_iter_* on CPU tensors and stub networks: past the refusal every one of them raises something else (a TypeError or
    RuntimeError for the CPU tensors, or an AttributeError of the stub), so a NotImplementedError with the message shows it came first."""
    net, dis = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    x, ids = torch.zeros(2, 34, 27), torch.zeros(2, 34, dtype=torch.int64)
    if which == "seq2seq":
        return pkg.train_iter_seq2seq(ARGS, 0, ids, [34, 34], x, net, bad(net))
    if which == "embed":
        return pkg.train_iter_embed(ARGS, 0, ids, torch.zeros(2, 36267), x, net, bad(net), "speech")
    s2g = pkg.speech2gesture
    g_opt, d_opt = (bad(net), good(dis)) if which == "s2g_generator" else (good(net), bad(dis))
    return s2g.train_iter_speech2gesture(ARGS, torch.zeros(2, 128, 70), x, net, dis, g_opt, d_opt, torch.nn.L1Loss())


WHO = {"seq2seq": "train_iter_seq2seq", "embed": "train_iter_embed", "s2g_generator": "train_iter_speech2gesture",
       "s2g_discriminator": "train_iter_speech2gesture"}


@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("which", sorted(WHO))
def test_train_iters_refuse_what_the_device_adam_cannot_honour(pkg, which, bad):
    with pytest.raises(NotImplementedError) as e:
        run(pkg, which, BAD[bad])
    assert str(e.value) == WHO[which] + MESSAGE


@pytest.mark.parametrize("which", sorted(WHO))
def test_a_plain_adam_gets_past_the_refusal(pkg, which):
    with pytest.raises(Exception) as e:
        run(pkg, which, good)
    assert not isinstance(e.value, NotImplementedError), e.value


def test_adopt_keeps_one_trainer_per_optimiser_and_network(pkg):
    adopt = pkg.optim.adopt
    net, other = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    opt = good(net)
    made = []

    def make(n):
        made.append(SimpleNamespace(net=n))
        return made[-1]
    tr, g = adopt(opt, "_t", "f", lambda: make(net), lambda t: t.net is net)
    assert tr is made[0] and opt._t is tr and g is opt.param_groups[0]
    assert adopt(opt, "_t", "f", lambda: make(net), lambda t: t.net is net)[0] is tr and len(made) == 1
    tr2, _ = adopt(opt, "_t", "f", lambda: make(other), lambda t: t.net is other)           # another network: a new trainer
    assert tr2 is made[1] and opt._t is tr2 and tr2.net is other
    opt.param_groups[0]["weight_decay"] = 1e-2                                                # set later: refused on the next call
    with pytest.raises(NotImplementedError):
        adopt(opt, "_t", "f", lambda: make(other), lambda t: t.net is other)
    assert len(made) == 2
