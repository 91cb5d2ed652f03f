"""The device Adams (torch.optim.Adam semantics, train.py:104-109): FusedAdam over a flat parameter slab, ParamAdam over a list of
parameters, and adopt(), which keeps a baseline's trainer on the torch optimiser its train_iter_* function is handed."""
import torch

from . import ops


class FusedAdam:
    """One launch per step for the whole network.  Same maths as torch.optim.Adam(lr, betas, eps=1e-8) without weight
    decay / amsgrad; the step counter lives on the device so a captured hipGraph replays correctly."""

    def __init__(self, module_or_engine, lr, betas=(0.5, 0.999), eps=1e-8):
        eng = getattr(module_or_engine, "engine", module_or_engine)
        self.engine = eng
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)

    @property
    def slab(self):
        return self.engine.slab.ensure()

    def zero_grad(self, set_to_none=False):
        self.slab.zero_grad()

    def step(self, counter_advanced=False):
        """counter_advanced: the device-side step counter was already incremented for this step (ops.iter_begin at the iteration's start)."""
        s = self.slab
        n = s.n_train                                  # frozen parameters sit behind the trainable prefix and are never stepped
        if not counter_advanced:
            ops.counter_inc(s.step)
        ops.adam_step(s.flat[:n], s.grad[:n], s.m[:n], s.v[:n], self.lr, self.betas[0], self.betas[1], self.eps, s.step)

    def state_dict(self):
        s = self.slab
        return {"step": int(s.step.item()), "exp_avg": s.m.clone(), "exp_avg_sq": s.v.clone(), "lr": self.lr,
                "betas": self.betas, "eps": self.eps, "names": list(s.names), "offsets": list(s.offsets)}

    def load_state_dict(self, sd):
        s = self.slab
        # the moments are flat images of the slab: they only mean something under the layout they were saved with (the order depends on
        # which parameters were frozen, e.g. freeze_wordembed)
        if "names" in sd and (list(sd["names"]) != list(s.names) or list(sd["offsets"]) != list(s.offsets)):
            raise ValueError("optimizer state was saved under a different parameter layout (different frozen set or network): "
                             f"{len(sd['names'])} tensors / {len(s.names)} here")
        assert sd["exp_avg"].numel() == s.m.numel(), (sd["exp_avg"].numel(), s.m.numel())
        s.m.copy_(sd["exp_avg"]); s.v.copy_(sd["exp_avg_sq"])
        s.step.fill_(int(sd["step"]))


class ParamAdam:
    """One tg_adam_step per parameter: torch.optim.Adam(lr, betas, eps) without weight decay / amsgrad over `params`, one moment pair per
    parameter, the step counter on the device.  A parameter whose .grad is None is skipped as torch.optim.Adam skips it: its value and its
    moments stay as they are (a zero gradient would still move it once its moments are non-zero); the counter advances all the same."""

    def __init__(self, params, lr, betas=(0.5, 0.999), eps=1e-8):
        self.params = list(params)
        self.m, self.v = [torch.zeros_like(p) for p in self.params], [torch.zeros_like(p) for p in self.params]
        self.step_dev = torch.zeros(1, device=self.params[0].device, dtype=torch.int32)
        self.set_hparams(lr, betas, eps)

    def set_hparams(self, lr, betas, eps):
        self.lr, self.betas, self.eps = lr, tuple(betas), eps

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def live_grads(self):
        """The gradients of the parameters that received one, each made contiguous in place on p.grad (what a clip between the backward
        and step() works on)."""
        grads = []
        for p in self.params:
            g = p.grad
            if g is None:
                continue
            if not g.is_contiguous():
                g = p.grad = g.contiguous()
            grads.append(g)
        return grads

    def step(self):
        ops.counter_inc(self.step_dev)
        lr, (b1, b2), eps, step = self.lr, self.betas, self.eps, self.step_dev
        for p, m, v in zip(self.params, self.m, self.v):
            g = p.grad
            if g is None:
                continue
            if not g.is_contiguous():
                g = p.grad = g.contiguous()
            ops.adam_step(p.data, g, m, v, lr, b1, b2, eps, step)


def adam_group(optim, who):
    """param_groups[0] of a torch optimiser whose hyper-parameters the device Adam can honour; anything else raises, before a tensor is
    touched: another optimiser class, several parameter groups, weight_decay, amsgrad."""
    g = optim.param_groups[0]
    if not isinstance(optim, torch.optim.Adam) or len(optim.param_groups) != 1 or g.get("weight_decay", 0) or g.get("amsgrad", False):
        raise NotImplementedError(f"{who} steps with the device Adam: pass a torch.optim.Adam with one parameter group, no weight_decay, no amsgrad")
    return g


def adopt(optim, attr, who, make, same):
    """-> (the trainer kept on `optim` under `attr`, optim.param_groups[0]).  The device Adam moments live in the trainer, so they go with
    the optimiser; make() builds a new one when there is none yet or same(trainer) is false (another network).  `optim` is a
    torch.optim.Adam whose hyper-parameters are used (read on every call, so schedules apply) and whose own step() and state are NOT;
    adam_group refuses the rest first, naming the calling function `who`."""
    g = adam_group(optim, who)
    tr = getattr(optim, attr, None)
    if tr is None or not same(tr):
        tr = make()
        setattr(optim, attr, tr)
    return tr, g
