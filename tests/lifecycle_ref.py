"""Shared by test_module_lifecycle_cpu.py / test_module_lifecycle_gpu.py (test infrastructure, not product code): the small
nets, the shapes, the ways user code writes weights, and a cache of oracle results.

The reference of every lifecycle assertion is oracle/unet_oracle.py evaluated on the model's state dict as it stands at
that moment; nothing here runs a HIP kernel."""
import torch

from oracle import unet_oracle as O
from util import gen, onehot_target, rel_err

SPECS = {"plain": O.NetSpec(n_blocks=2), "sp": O.NetSpec(in_ch=2, out_ch=3, n_blocks=2, head="sp")}
# (N, D, H, W).  A: the decoder's top level (coarse 16^3, 32 -> 8 padded channels) takes the fused up-convolution in fp32 and
# in 16-bit, and the full-resolution 8 -> 8 convolution the W >= 32 pair layout.  B: W = 24 -- layout 0, and a coarse W of 12
# is below the fused kernels' 16: the same layers run unfused, from the OTHER cache.  C: fused again, non-cubic.
SHAPES = {"A": (1, 32, 32, 32), "B": (2, 16, 32, 24), "C": (1, 16, 16, 48)}
# every mutation writes: an encoder conv, the 8 -> 8 pair-layout conv, both ConvTranspose3d (the fused top level, the unfused
# bottom level) with their biases, and the convs after them
TARGETS = ["d_blocks.1.block.0.weight", "d_blocks.0.block.3.weight", "u_blocks.1.block.0.weight", "u_blocks.1.block.0.bias",
           "u_blocks.1.block.1.weight", "u_blocks.0.block.0.weight", "u_blocks.0.block.0.bias", "u_blocks.0.block.1.weight"]
BN_LAYERS = ["d_blocks.1.block.1", "u_blocks.1.block.2", "u_blocks.1.block.5"]
SEPARATION = 1e-2          # old-weight vs new-weight oracle outputs, of max |ref|: 100 x the fp32 output gate


def _ctunet():
    import ctunet_amd
    return ctunet_amd


class SmallSP(_ctunet().UNetSP):
    """UNetSP's two-output head on the two-block net."""

    def __init__(self, use_checkpoint=False):
        _ctunet().UNet.__init__(self, input_channels=2, out_channels=3, n_blocks=2, use_checkpoint=use_checkpoint)
        self._set_head()


def make_net(kind="plain", use_checkpoint=False, seed=0):
    torch.manual_seed(seed)
    if kind == "sp":
        return SmallSP(use_checkpoint)
    return _ctunet().UNet(n_blocks=2, use_checkpoint=use_checkpoint)


def make_input(kind, shape, seed=0):
    n, d, h, w = SHAPES[shape]
    return torch.randn(n, SPECS[kind].in_ch, d, h, w, generator=gen(100 + seed + sum(map(ord, shape))))


def make_targets(kind, shape):
    n, d, h, w = SHAPES[shape]
    return [onehot_target((n, 2, d, h, w), 4321 + i, 0.2) for i in range(2 if kind == "sp" else 1)]


def loss_of(kind, out, targets, which="all"):
    """The handler losses of the oracle, on whatever device / dtype `out` and `targets` live.  which="first": only the first
    output of a two-output head enters the loss."""
    if kind == "sp" and which == "all":
        return O.loss_double(out, targets, 1.0, 1.0)[0]
    return O.loss_single(out[0] if kind == "sp" else out, targets[0], 1.0, 1.0)[0]


def snapshot(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


# ------------------------------------------------------------------------------------------------ oracle cache
class OracleCache:
    """Oracle results per (state dict contents, shape, mode): a test asks for the same state several times (separation of a
    mutation, then the checks on it)."""

    def __init__(self, kind):
        self.kind, self.spec, self._c = kind, SPECS[kind], {}
        self.x = {s: make_input(kind, s) for s in SHAPES}
        self.t = {s: make_targets(kind, s) for s in SHAPES}

    @staticmethod
    def _fp(sd):
        return hash(b"".join(v.detach().cpu().contiguous().numpy().tobytes() for _, v in sorted(sd.items())))

    def eval_out(self, sd, shape, autocast=None):
        """Eval-mode outputs (a tuple); autocast=dtype: the same forward under torch.autocast (the 16-bit yardstick)."""
        key = (self._fp(sd), shape, "eval", autocast)
        if key not in self._c:
            with torch.no_grad(), torch.autocast("cpu", dtype=autocast or torch.bfloat16, enabled=autocast is not None):
                o = O.forward(self.spec, sd, self.x[shape], training=False)
            self._c[key] = tuple(a.float() for a in (o if isinstance(o, tuple) else (o,)))
        return self._c[key]

    def train(self, sd, shape, which="all", fp64=True, autocast=None):
        """One train-mode step on `sd` (not modified).  Returns a dict: outs, loss, g32, dx32, (loss64, g64, dx64), post
        (the state dict after the step's running-statistics update), post2 (after the second update a checkpointed step
        makes: every live BatchNorm twice, the dead centre block once) and, with autocast=dtype, `ac`: the same step of the
        oracle under torch.autocast -- the suite's yardstick for the 16-bit path (tests/test_lowp_gpu.py)."""
        key = (self._fp(sd), shape, "train", which, fp64, autocast)
        if key in self._c:
            return self._c[key]
        x, t = self.x[shape], self.t[shape]

        def run(dt, state):
            s = {k: (v.to(dt, copy=True) if v.is_floating_point() else v.clone()) for k, v in state.items()}     # (the step moves s's buffers)
            tt = [a.to(dt) for a in t]
            out, loss, g, dx = O.grads(self.spec, s, x.to(dt), lambda o: loss_of(self.kind, o, tt, which), training=True)
            return (out if isinstance(out, tuple) else (out,)), loss, g, dx, s
        outs, loss, g32, dx32, post = run(torch.float32, sd)
        r = {"outs": [o.detach() for o in outs], "loss": loss.item(), "g32": g32, "dx32": dx32, "post": post}
        with torch.no_grad():
            post2 = {k: v.clone() for k, v in post.items()}
            O.forward(self.spec, post2, x, training=True)
            r["post2"] = {k: (post[k] if k.startswith("cblock.") else v) for k, v in post2.items()}
        if fp64:
            _, l64, r["g64"], r["dx64"], _ = run(torch.float64, sd)
            r["loss64"] = l64.item()
        if autocast is not None:
            s = {k: v.clone() for k, v in sd.items()}
            with torch.autocast("cpu", dtype=autocast):
                out, l, g, dx = O.grads(self.spec, s, x, lambda o: loss_of(
                    self.kind, tuple(a.float() for a in o) if isinstance(o, tuple) else o.float(), t, which), training=True)
            r["ac"] = ([o.detach() for o in (out if isinstance(out, tuple) else (out,))], l.item(), g, dx)
        self._c[key] = r
        return r

    def separation(self, sd_old, sd_new, shape):
        """(eval, train) distance of the oracle's outputs on the two states, of max |ref|."""
        e = max(rel_err(a, b) for a, b in zip(self.eval_out(sd_old, shape), self.eval_out(sd_new, shape)))
        t = max(rel_err(a, b) for a, b in zip(self.train(sd_old, shape, fp64=False)["outs"], self.train(sd_new, shape, fp64=False)["outs"]))
        return e, t


# ------------------------------------------------------------------------------------------------ weight mutations
def _mult(p, k, j):
    """Per-element multiplier of mutation k for the j-th target: random sign, magnitude in [0.5, 1.5].  (A plain factor is
    invisible in train mode -- the BatchNorm behind each conv divides it out -- and a sign flip undoes itself when applied
    twice, so neither tells the last state from the one before.)"""
    g = gen(7919 * (k + 1) + j)
    sign = (torch.rand(p.shape, generator=g) < 0.5).float() * 2 - 1
    return (sign * (0.5 + torch.rand(p.shape, generator=g))).to(p.device)


def _targets(net):
    P = dict(net.named_parameters())
    return [(j, P[n_]) for j, n_ in enumerate(TARGETS)]


def _fake_grads(net, k):
    """Gradients of the parameters' own size, so that ONE optimizer step moves every weight by about its magnitude."""
    for j, (_, p) in enumerate(net.named_parameters()):
        g = torch.randn(p.shape, generator=gen(104729 * (k + 1) + j)).to(p.device)
        p.grad = g * p.detach().abs().mean().clamp_min(1e-3)


def m_no_grad_mul(net, k):
    with torch.no_grad():
        for j, p in _targets(net):
            p.mul_(_mult(p, k, j))


def m_detach_mul(net, k):
    for j, p in _targets(net):
        p.detach().mul_(_mult(p, k, j))


def m_data_mul(net, k):
    for j, p in _targets(net):
        p.data.mul_(_mult(p, k, j))


def m_data_copy(net, k):
    for j, p in _targets(net):
        p.data.copy_(p.detach() * _mult(p, k, j))


def m_data_assign(net, k):
    for j, p in _targets(net):
        p.data = p.detach() * _mult(p, k, j)


def _mutated_sd(net, k):
    sd = {n_: v.detach().clone() for n_, v in net.state_dict().items()}
    for j, n_ in enumerate(TARGETS):
        sd[n_] = sd[n_] * _mult(sd[n_], k, j)
    return sd


def m_load_state_dict(net, k):
    net.load_state_dict(_mutated_sd(net, k))


def m_load_state_dict_assign(net, k):
    net.load_state_dict(_mutated_sd(net, k), assign=True)


def m_init(net, k):
    torch.manual_seed(1000 + k)
    for j, p in _targets(net):
        if p.dim() == 5:
            torch.nn.init.kaiming_uniform_(p, a=5 ** 0.5)
        else:
            torch.nn.init.uniform_(p, -0.2, 0.2)


def m_vector_to_parameters(net, k):
    ps = [p for _, p in _targets(net)]
    vec = torch.nn.utils.parameters_to_vector(ps).detach()
    torch.nn.utils.vector_to_parameters(vec * torch.cat([_mult(p, k, j).flatten() for j, p in enumerate(ps)]), ps)


def _sgd(foreach):
    def step(net, k):
        _fake_grads(net, k)
        torch.optim.SGD(net.parameters(), lr=1.0, foreach=foreach).step()
        net.zero_grad(set_to_none=True)
    return step


def m_adam_fused(net, k):
    _fake_grads(net, k)
    torch.optim.Adam(net.parameters(), lr=0.05, fused=True).step()       # (first Adam step: every entry moves by lr)
    net.zero_grad(set_to_none=True)


def m_sgd_fused(net, k):
    _fake_grads(net, k)
    torch.optim.SGD(net.parameters(), lr=1.0, fused=True).step()
    net.zero_grad(set_to_none=True)


def m_project_adam(net, k):
    from ctunet_amd import optim
    _fake_grads(net, k)
    optim.Adam(net.parameters(), lr=0.05, amsgrad=True).step()
    net.zero_grad(set_to_none=True)


# name -> (function(net, k), p._version moves, p.data_ptr() moves (None: the Parameter object itself is replaced),
#          neither moves: the caches cannot see the write and INTEGRATION.md asks for invalidate_packed_weights())
PATHWAYS = {
    "no_grad_mul": (m_no_grad_mul, True, False, False),
    "detach_mul": (m_detach_mul, True, False, False),
    "data_mul": (m_data_mul, False, False, True),
    "data_copy": (m_data_copy, False, False, True),
    "data_assign": (m_data_assign, False, True, False),
    "load_state_dict": (m_load_state_dict, True, False, False),
    "load_state_dict_assign": (m_load_state_dict_assign, None, None, False),
    "init": (m_init, True, False, False),
    "vector_to_parameters": (m_vector_to_parameters, False, True, False),
    "sgd_foreach": (_sgd(True), True, False, False),
    "sgd_single": (_sgd(False), True, False, False),
    # torch's fused optimizers write through tensor-list kernels that leave the version counters alone (on the CPU and on
    # the GPU build alike): as invisible as a .data write
    "adam_fused": (m_adam_fused, False, False, True),
    "sgd_fused": (m_sgd_fused, False, False, True),
    "project_adam": (m_project_adam, True, False, False),       # (GPU only: one fused HIP launch)
}


def m_batchnorm_data(net, k):
    """BatchNorm gamma / beta / running statistics written in place through .data."""
    T = dict(net.named_parameters())
    T.update(dict(net.named_buffers()))
    for j, bn in enumerate(BN_LAYERS):
        g = gen(31 * (k + 1) + j)
        c = T[bn + ".weight"].numel()
        r = lambda: torch.rand(c, generator=g).to(T[bn + ".weight"].device)
        T[bn + ".weight"].data.mul_(-(0.5 + r()))
        T[bn + ".bias"].data.add_(r() - 0.3)
        T[bn + ".running_mean"].data.add_(r() - 0.5)
        T[bn + ".running_var"].data.mul_(0.5 + 2 * r())
