"""Plain-torch restatement of the rules of ``ctu_sgd`` / ``ctu_rmsprop`` (include/ctunet_hip.h): functions over tensors
in the tensors' own dtype and in the rules' own order of operations, with no ``torch.optim`` inside.  The caller owns what
the kernels read from the device: ``skip`` (the overflow flag: nothing is written) and ``first`` (SGD: this is the first
APPLIED step, the device counter reads 1 after its increment).  Everything is updated in place."""
import itertools

import torch

# the option grids of the issue: mu in {0, 0.9}, delta in {0, 0.3}, nesterov, lambda in {0, 0.01}, maximize, centered
SGD_GRID = [dict(momentum=mu, dampening=d, nesterov=nv, weight_decay=wd, maximize=mx)
            for mu, d, nv, wd, mx in itertools.product((0.0, 0.9), (0.0, 0.3), (False, True), (0.0, 0.01), (False, True))
            if not (nv and (mu == 0.0 or d != 0.0))]              # (torch refuses Nesterov without momentum / with dampening)
RMS_GRID = [dict(momentum=mu, centered=c, weight_decay=wd, maximize=mx)
            for mu, c, wd, mx in itertools.product((0.0, 0.9), (False, True), (0.0, 0.01), (False, True))]


def grid_id(kw):
    return "-".join(f"{k[:3]}{v:g}" if isinstance(v, float) else (k[:3] if v else f"no{k[:3]}") for k, v in kw.items())


def _grad(p, g, coef, weight_decay, maximize):
    if coef is not None:
        g = coef * g
    if maximize:
        g = -g
    if weight_decay != 0:
        g = g + weight_decay * p
    return g


@torch.no_grad()
def sgd_step(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False, coef=None,
             first=False, skip=False):
    """p, buf in place (buf: None when momentum == 0)."""
    if skip:
        return
    g = _grad(p, g, coef, weight_decay, maximize)
    if momentum != 0:
        if first:
            buf.copy_(g)
        else:
            buf.copy_(momentum * buf + (1 - dampening) * g)
        g = g + momentum * buf if nesterov else buf
    p.copy_(p - lr * g)


@torch.no_grad()
def rmsprop_step(p, g, sq, buf, ga, lr, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False,
                 maximize=False, coef=None, skip=False):
    """p, sq, buf, ga in place (buf: None when momentum == 0, ga: None when not centered)."""
    if skip:
        return
    g = _grad(p, g, coef, weight_decay, maximize)
    sq.copy_(alpha * sq + (1 - alpha) * g * g)
    if centered:
        ga.copy_(ga + (1 - alpha) * (g - ga))
        avg = torch.sqrt(sq - ga * ga) + eps
    else:
        avg = torch.sqrt(sq) + eps
    if momentum > 0:
        buf.copy_(momentum * buf + g / avg)
        p.copy_(p - lr * buf)
    else:
        p.copy_(p - lr * (g / avg))


class Runner:
    """Steps a list of tensors with one of the two rules, keeping their state and the counters the kernels keep on the
    device (``steps``: applied steps).  ``grads[i]`` None: that tensor is skipped and gets no state."""

    def __init__(self, rule, params, lr, **kw):
        assert rule in ("sgd", "rmsprop")
        self.rule, self.params, self.lr, self.kw = rule, params, lr, kw
        self.state = [None] * len(params)
        self.steps = 0

    def step(self, grads, coef=None, skip=False):
        if skip:
            return
        self.steps += 1
        mu = self.kw.get("momentum", 0.0)
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                continue
            if self.state[i] is None:
                z = lambda: torch.zeros_like(p)
                self.state[i] = dict(momentum_buffer=z() if mu != 0 else None) if self.rule == "sgd" else \
                    dict(square_avg=z(), momentum_buffer=z() if mu > 0 else None,
                         grad_avg=z() if self.kw.get("centered") else None)
            st = self.state[i]
            if self.rule == "sgd":
                sgd_step(p, g, st["momentum_buffer"], self.lr, coef=coef, first=self.steps == 1, **self.kw)
            else:
                rmsprop_step(p, g, st["square_avg"], st["momentum_buffer"], st["grad_avg"], self.lr, coef=coef, **self.kw)
