"""fp64 torch restatement of the Gabor and Sarf activations (csrc/param_act.h's formulas, i.e.
gaborf/gabor.py:8-64 and sarf/activation.py:63-65) shared by test_gabor_sarf_logic.py and
test_gpu_gabor_sarf.py.  Everything is computed in the dtype of its inputs."""
import torch

KINDS = {"gaborf": 1, "sarf": 2}                                   # NERF_ACT_GABOR, NERF_ACT_SARF
PARAMS = {"gaborf": ("inv_standard_deviation", "spread"), "sarf": ("frequency",)}
INIT = {"gaborf": (0.0, 2.0), "sarf": (0.5, 2.0)}                  # the families' main.py init ranges


def gabor_fwd(z, s, p):
    v = s * s + 1e-6
    return torch.exp((-(z * z)) * v) * torch.cos(p * z)


def gabor_bwd(g, z, s, p):
    """The reference's hand-written GaborActivation.backward: (dz, ds, dp)."""
    v = s * s + 1e-6
    go = -torch.exp(-v * z * z) * g
    c, sn = torch.cos(p * z), torch.sin(p * z)
    dz = go * (2 * c * v * z + p * sn)
    dv = (go * z * z * c).sum(0)
    dp = (go * z * sn).sum(0)
    return dz, dv * (2 * s), dp


def sarf_fwd(z, f):
    u = (z.abs() + 1e-4) ** 2
    return torch.cos(f / (u + 1 / (f * f))) * torch.exp(-u)


def sarf_bwd(g, z, f):
    """What autograd gives the reference: (dz, df); sign(+-0) = 0."""
    t = z.abs() + 1e-4
    u = t * t
    q = u + 1 / (f * f)
    a = f / q
    e = torch.exp(-u)
    dz = g * (e * (torch.sin(a) * f / (q * q) - torch.cos(a))) * (2 * t * torch.sign(z))
    df = (g * (-torch.sin(a) * e * (1 / q + 2 / (f * f * q * q)))).sum(0)
    return dz, df


def act_fwd(family, z, *params):
    return gabor_fwd(z, *params) if family == "gaborf" else sarf_fwd(z, *params)


def act_bwd(family, g, z, *params):
    """(dz, parameter gradients...)"""
    return gabor_bwd(g, z, *params) if family == "gaborf" else sarf_bwd(g, z, *params)


class TorchAct(torch.nn.Module):
    """The activation as a plain torch module over the restated forward (autograd backward)."""

    def __init__(self, family, params):
        super().__init__()
        self.family = family
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in params])

    def forward(self, z):
        return act_fwd(self.family, z, *self.ps)


def modules(family):
    """(module, activation class) of the family in nerf_amd."""
    if family == "gaborf":
        from nerf_amd import model_gaborf as m
        return m, m.GaborAct
    from nerf_amd import model_sarf as m
    return m, m.SarfAct
