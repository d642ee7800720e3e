"""Golden data of the GaborF and SARF field networks, produced by the reference's own modules
(gaborf/gabor.py, model_radiance.py, model_proposal.py; sarf/activation.py, model_radiance.py,
model_proposal.py), imported from their directories and run eagerly on the CPU.  Writes
gaborf.npz and sarf.npz next to this file.  Usage:

    NERF_REFERENCE=/path/to/nerf-experiments python tests/golden/make_golden_gabor_sarf.py

sarf/ builds its Sequentials under ``th.compile``; here ``th.compile`` is rebound, before the
import, to an eager wrapper that keeps the wrapped module under ``_orig_mod`` as the real one does,
so the state_dict key names are the reference's.

Contents (mirroring gen_garf of make_golden.py), per family:
  network part   pos [257, 3] in [-2, 2), unit dir; th.manual_seed(0) construction with the
                 family's main.py init range; state_dict key names and checksums, outputs, upstream
                 gradients, dpos / ddir, per-parameter gradient sums and (<= 1024 elements) gradients
  activation     z = randn(64, 48) * 3 with z[0, :4] = [0, -0, 30, -1e-3]; parameters as below;
                 y, gy, dz and the parameter gradients in fp32 (the reference as it runs) and from
                 the same module cast to fp64 (``*.f64`` keys)
"""
import importlib
import math
import os
import sys

import numpy as np
import torch as th
import torch.nn as nn

REF = os.environ.get("NERF_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
# Full gradients are stored for parameters up to this size: every bias and activation parameter
# (those of the 1024- and 512-wide layers included, which take the kernels' column-block route) and
# the 256 x 3 colour head; larger ones are pinned by their gradient sums (gen_garf stores up to 4096).
# Sizes: gaborf.npz 208 KB, sarf.npz 185 KB against garf.npz's 151 KB.  98 KB of each is the
# activation-alone block (six 64 x 48 fp32 / fp64 arrays of random data, which do not compress) and
# 26 KB the networks' inputs, outputs and input gradients; Gabor has two parameters per channel.
FULL_GRAD_MAX = 1024


class _Eager(nn.Module):
    """Stands in for th.compile's OptimizedModule: same attribute name, eager forward."""

    def __init__(self, mod):
        super().__init__()
        self._orig_mod = mod

    def forward(self, *a, **k):
        return self._orig_mod(*a, **k)


th.compile = lambda m=None, *a, **k: _Eager(m) if isinstance(m, nn.Module) else m


def _import_from(subdir, names):
    for n in names:
        sys.modules.pop(n, None)
    sys.path.insert(0, os.path.join(REF, subdir))
    try:
        return [importlib.import_module(n) for n in names]
    finally:
        sys.path.pop(0)


def f32(t):
    return t.detach().to(th.float32).numpy()


def f64(t):
    return t.detach().to(th.float64).numpy()


def networks(out, rad_cls, prop_cls, lo, hi, g):
    N = 257
    pos = th.rand(N, 3, generator=g) * 4 - 2
    d = th.randn(N, 3, generator=g)
    d = d / th.linalg.vector_norm(d, dim=1, keepdim=True)
    out["pos"], out["dir"] = f32(pos), f32(d)
    th.manual_seed(0)
    rad = rad_cls(lo, hi)
    th.manual_seed(0)
    prop = prop_cls(lo, hi)
    for name, m in (("radiance", rad), ("proposal", prop)):
        out[f"{name}.keys"] = np.array(list(m.state_dict().keys()))
        for k, v in m.state_dict().items():
            out[f"{name}.sdsum.{k}"] = np.array([v.double().sum().item(), v.double().abs().sum().item()])
        p = pos.clone().requires_grad_(True)
        dd = d.clone().requires_grad_(True)
        if name == "radiance":
            rgb, dens = m.forward(p, dd)
            gc = th.randn(N, 3, generator=g)
            gd = th.randn(N, generator=g)
            ((rgb * gc).sum() + (dens * gd).sum()).backward()
            out[f"{name}.rgb"], out[f"{name}.density"] = f32(rgb), f32(dens)
            out[f"{name}.gc"], out[f"{name}.gd"] = f32(gc), f32(gd)
            out[f"{name}.ddir"] = f32(dd.grad)
        else:
            dens = m.forward(p)
            gd = th.randn(dens.shape, generator=g)
            (dens * gd).sum().backward()
            out[f"{name}.density"], out[f"{name}.gd"] = f32(dens), f32(gd)
        out[f"{name}.dpos"] = f32(p.grad)
        for k, prm in m.named_parameters():
            if prm.numel() <= FULL_GRAD_MAX:
                out[f"{name}.grad.{k}"] = f32(prm.grad)
            out[f"{name}.gradsum.{k}"] = np.array([prm.grad.double().sum().item(),
                                                   prm.grad.double().abs().sum().item()])


def activation(out, make_act, params, g, z):
    """params: {attribute: fp32 value}; fp32 run and the same module in fp64."""
    gy = th.randn(z.shape, generator=g)
    out["act.z"], out["act.gy"] = f32(z), f32(gy)
    for k, v in params.items():
        out[f"act.{k}"] = f32(v)
    for dt, suffix, cv in ((th.float32, "", f32), (th.float64, ".f64", f64)):
        act = make_act().to(dt)
        with th.no_grad():
            for k, v in params.items():
                getattr(act, k).copy_(v.to(dt))
        zz = z.to(dt).clone().requires_grad_(True)
        y = act(zz)
        (y * gy.to(dt)).sum().backward()
        out[f"act.y{suffix}"], out[f"act.dz{suffix}"] = cv(y), cv(zz.grad)
        for k in params:
            out[f"act.d_{k}{suffix}"] = cv(getattr(act, k).grad)


def act_input(g):
    z = th.randn(64, 48, generator=g) * 3
    z[0, :4] = th.tensor([0.0, -0.0, 30.0, -1e-3])
    return z


def gen_gaborf():
    gabor_m, rad_m, prop_m = _import_from("gaborf", ["gabor", "model_radiance", "model_proposal"])
    g = th.Generator().manual_seed(17)
    out = {}
    networks(out, rad_m.RadianceNetwork, prop_m.ProposalNetwork, 0.0, 2.0, g)      # gaborf/main.py:144-145
    z = act_input(g)
    s = th.rand(48, generator=g) * 2
    s[0] = 0.0
    spread = th.rand(48, generator=g) * 2 * math.pi
    activation(out, lambda: gabor_m.GaborAct(48), {"inv_standard_deviation": s, "spread": spread}, g, z)
    np.savez_compressed(os.path.join(OUT, "gaborf.npz"), **out)


def gen_sarf():
    act_m, rad_m, prop_m = _import_from("sarf", ["activation", "model_radiance", "model_proposal"])
    g = th.Generator().manual_seed(18)
    out = {}
    networks(out, rad_m.RadianceNetwork, prop_m.ProposalNetwork, 0.5, 2.0, g)      # sarf/main.py:29-30
    z = act_input(g)
    f = th.rand(48, generator=g) * 1.5 + 0.5
    f[5] = -f[5]
    activation(out, lambda: act_m.SarfAct(48, 0.5, 2.0), {"frequency": f}, g, z)
    np.savez_compressed(os.path.join(OUT, "sarf.npz"), **out)


if __name__ == "__main__":
    gen_gaborf()
    gen_sarf()
    for n in ("gaborf.npz", "sarf.npz"):
        print(n, os.path.getsize(os.path.join(OUT, n)), "bytes")
