"""Golden data of the SIREN networks, produced by the reference's own modules (nerf-siren/
linear_sine.py, nerf_model.py, model.py), imported from their directory with import stubs for the
absent pytorch_lightning / data_module (as make_golden.py does) and run eagerly on the CPU.  Writes
siren.npz next to this file.  Usage:

    NERF_REFERENCE=/path/to/nerf-experiments python tests/golden/make_golden_siren.py

The 530,695 weights of a NerfModel are not stored: they come from th.manual_seed(0) at construction
(the fixture holds every tensor's (sum, abs-sum) digest).  Likewise the [257, 259] input of the
second LinearSine case and the upstream gradients come from tests/_siren_ref.py's recipes, with
their digests here.

Contents:
  ls0 / ls1   LinearSine(3 -> 256, scale=32, first_layer=True) and LinearSine(259 -> 256, scale =
              [1 x 256, 32, 32, 32]) on x [257, in] under the upstream gradient upstream(256):
              y and dx on the stored rows with their fp64 row / column sums, dW as digest + sampled
              entries, db
  model       NerfModel(32): pos [257, 3] uniform in [-1, 1), unit dir, loss = sum_m w_m (density_m +
              sum rgb_m), w = linspace(0.5, 1.5): density, rgb, dpos, ddir; per parameter / buffer the
              digest of its value, per parameter the digest, maximum and sampled entries of its gradient
  siren       NerfSiren(near=1/3, far=1, fine=32, coarse=16) on 64 rays with _sample_t_coarse replaced
              by the stored t_coarse: rgb_fine, rgb_coarse, t_fine
  dev.*       the error yardstick: every stored tensor evaluated two more ways, in fp64 and with every
              Linear product (forward and both backward GEMMs) replaced by the 3 x bf16 split
              restatement hi*hi + hi*lo + lo*hi; per tensor [max|fp32 - fp64|, max|split - fp64|,
              max|fp64|].  The generator refuses inputs for which the split restatement changes a
              ray's fine-sample counts.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch as th

REF = os.environ.get("NERF_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import _siren_ref as R  # noqa: E402


def _install_stubs():
    pl = types.ModuleType("pytorch_lightning")

    class LightningModule(th.nn.Module):
        def save_hyperparameters(self, *a, **k):
            pass

        @property
        def device(self):
            return th.device("cpu")

        def log(self, *a, **k):
            pass

    pl.LightningModule = LightningModule
    sys.modules["pytorch_lightning"] = pl
    dm = types.ModuleType("data_module")
    dm.DatasetOutput = tuple
    sys.modules["data_module"] = dm


def _import_siren():
    names = ["linear_sine", "nerf_model", "model"]
    for n in names:
        sys.modules.pop(n, None)
    sys.path.insert(0, os.path.join(REF, "nerf-siren"))
    try:
        return [importlib.import_module(n) for n in names]
    finally:
        sys.path.pop(0)
        for n in names:
            sys.modules.pop(n, None)


# ------------------------------------------------------------------ the 3 x bf16 split restatement
def _split(a):
    hi = a.to(th.bfloat16).to(a.dtype)
    return hi, (a - hi).to(th.bfloat16).to(a.dtype)


def _mm3(a, b):
    ah, al = _split(a)
    bh, bl = _split(b)
    return ah @ bh + ah @ bl + al @ bh


class _SplitLinear(th.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        y = _mm3(x, w.t())
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return _mm3(g, w), _mm3(g.t(), x), g.sum(dim=0)


_F_LINEAR = th.nn.functional.linear


class _Evaluation:
    """One of the three ways a module is evaluated: fp32 as it runs, fp64, or fp32 with the split GEMMs."""

    def __init__(self, how):
        self.how = how
        self.dtype = th.float64 if how == "f64" else th.float32

    def __enter__(self):
        th.set_default_dtype(self.dtype)
        if self.how == "split":
            th.nn.functional.linear = lambda x, w, b=None: _SplitLinear.apply(x, w, b)
        return self

    def __exit__(self, *a):
        th.nn.functional.linear = _F_LINEAR
        th.set_default_dtype(th.float32)


def _three_ways(run):
    """run(dtype) -> {name: tensor}; returns the fp32 results and the dev.* records."""
    res = {}
    for how in ("f32", "f64", "split"):
        with _Evaluation(how) as e:
            res[how] = {k: v.detach().double() for k, v in run(e.dtype).items()}
    dev = {k: np.array([(res["f32"][k] - v).abs().max().item(), (res["split"][k] - v).abs().max().item(),
                        v.abs().max().item()]) for k, v in res["f64"].items()}
    return res, dev


def _store_rows(out, key, t):
    """A [257, n] tensor: the stored rows and every row's / column's fp64 sum."""
    out[key] = t[R.stored_rows()].to(th.float32).numpy()
    out[key + ".rowsum"] = t.double().sum(dim=1).numpy()
    out[key + ".colsum"] = t.double().sum(dim=0).numpy()


def _store_grad(out, key, g):
    out[key + ".digest"] = np.array(R.digest(g))
    out[key + ".max"] = np.array(g.abs().max().item())
    out[key + ".sample"] = g.reshape(-1)[R.sample_idx(g.numel())].to(th.float32).numpy()


# ------------------------------------------------------------------------------------ the parts
def gen_linear_sine(out, ls_mod):
    for key, k, n, first in R.LS_CASES:
        x32 = R.linear_sine_input(key, k)
        gy32 = R.upstream(n)
        out[f"{key}.x.digest"] = np.array(R.digest(x32))
        out[f"{key}.gy.digest"] = np.array(R.digest(gy32))
        if k <= 4:
            out[f"{key}.x"] = x32.numpy()

        def run(dtype):
            th.set_default_dtype(th.float32)   # construction is the reference's fp32 one in every evaluation
            th.manual_seed(0)
            m = ls_mod.LinearSine(k, n, scale=R.linear_sine_scale(key), first_layer=first)
            th.set_default_dtype(dtype)
            m = m.to(dtype)
            x = x32.clone().to(dtype).requires_grad_(True)
            y = m(x)
            (y * gy32.to(dtype)).sum().backward()
            return {"y": y, "dx": x.grad, "dW": m.linear.weight.grad, "db": m.linear.bias.grad,
                    "weight": m.linear.weight, "bias": m.linear.bias, "scale": m.scale}

        res, dev = _three_ways(run)
        r = res["f32"]
        _store_rows(out, f"{key}.y", r["y"])
        _store_rows(out, f"{key}.dx", r["dx"])
        _store_grad(out, f"{key}.dW", r["dW"])
        out[f"{key}.db"] = r["db"].to(th.float32).numpy()
        for p in ("weight", "bias", "scale"):
            out[f"{key}.sd.{p}"] = np.array(R.digest(r[p]))
        for t in ("y", "dx", "dW", "db"):
            out[f"dev.{key}.{t}"] = dev[t]


def gen_model(out, nm_mod):
    g = th.Generator().manual_seed(22)
    pos32 = th.rand(R.ROWS, 3, generator=g) * 2 - 1
    d32 = th.randn(R.ROWS, 3, generator=g)
    d32 = d32 / th.linalg.vector_norm(d32, dim=1, keepdim=True)
    w32 = th.linspace(0.5, 1.5, R.ROWS)
    out["model.pos"], out["model.dir"], out["model.w"] = pos32.numpy(), d32.numpy(), w32.numpy()
    names = {}

    def run(dtype):
        th.set_default_dtype(th.float32)       # construction is the reference's fp32 one in every evaluation
        th.manual_seed(0)
        m = nm_mod.NerfModel(32)
        th.set_default_dtype(dtype)
        m = m.to(dtype)
        names["keys"] = list(m.state_dict().keys())
        names["params"] = [k for k, _ in m.named_parameters()]
        pos = pos32.clone().to(dtype).requires_grad_(True)
        d = d32.clone().to(dtype).requires_grad_(True)
        density, rgb = m(pos, d)
        (w32.to(dtype) * (density + rgb.sum(dim=1))).sum().backward()
        r = {"density": density, "rgb": rgb, "dpos": pos.grad, "ddir": d.grad}
        r.update({f"sd.{k}": v for k, v in m.state_dict().items()})
        r.update({f"grad.{k}": p.grad for k, p in m.named_parameters()})
        return r

    res, dev = _three_ways(run)
    r = res["f32"]
    out["model.keys"] = np.array(names["keys"])
    out["model.params"] = np.array(names["params"])
    out["model.shapes"] = np.array([(list(r[f"sd.{k}"].shape) + [0, 0])[:2] for k in names["keys"]])
    for t in ("density", "rgb", "dpos", "ddir"):
        out[f"model.{t}"] = r[t].to(th.float32).numpy()
        out[f"dev.model.{t}"] = dev[t]
    for k in names["keys"]:
        out[f"model.sd.{k}"] = np.array(R.digest(r[f"sd.{k}"]))
    for k in names["params"]:
        _store_grad(out, f"model.grad.{k}", r[f"grad.{k}"])
        out[f"dev.model.grad.{k}"] = dev[f"grad.{k}"]


def gen_siren(out, model_mod):
    g = th.Generator().manual_seed(23)
    B, near, far, fine, coarse = 64, 1 / 3, 1.0, 32, 16
    o32 = th.randn(B, 3, generator=g)
    o32 = 0.3 * o32 / th.linalg.vector_norm(o32, dim=1, keepdim=True)
    d32 = th.randn(B, 3, generator=g)
    d32 = d32 / th.linalg.vector_norm(d32, dim=1, keepdim=True)
    interval = (far - near) / coarse
    t32 = th.linspace(near, far - interval, coarse).unsqueeze(0).repeat(B, 1) + th.rand(B, coarse, generator=g) * interval
    out["siren.origins"], out["siren.dirs"], out["siren.t_coarse"] = o32.numpy(), d32.numpy(), t32.numpy()
    out["siren.args"] = np.array([near, far, fine, coarse])

    def run(dtype):
        th.set_default_dtype(th.float32)
        th.manual_seed(0)
        m = model_mod.NerfSiren(near, far, fine, coarse)
        th.set_default_dtype(dtype)
        m = m.to(dtype)
        m._sample_t_coarse = lambda batch_size: t32.to(dtype).clone()
        kept = {}
        sample_fine = m._sample_t_fine

        def keep_fine(*a, **k):
            kept["t_fine"] = sample_fine(*a, **k)
            return kept["t_fine"]
        m._sample_t_fine = keep_fine
        with th.no_grad():
            rgb_fine, rgb_coarse = m(o32.to(dtype), d32.to(dtype))
        return {"rgb_fine": rgb_fine, "rgb_coarse": rgb_coarse, "t_fine": kept["t_fine"]}

    res, dev = _three_ways(run)
    # a changed fine-sample count moves a ray's samples by a fraction of a coarse bin (>= 1e-3 here);
    # rounding alone moves them by ~1e-7.  The split restatement must change no ray's counts.
    moved = (res["split"]["t_fine"] - res["f32"]["t_fine"]).abs().amax(dim=1)
    if (moved > 1e-4).any() or ((res["f64"]["t_fine"] - res["f32"]["t_fine"]).abs() > 1e-4).any():
        raise SystemExit("gen_siren: the fine-sample counts depend on the evaluation for these inputs; pick another seed")
    for t in ("rgb_fine", "rgb_coarse", "t_fine"):
        out[f"siren.{t}"] = res["f32"][t].to(th.float32).numpy()
        out[f"dev.siren.{t}"] = dev[t]


if __name__ == "__main__":
    _install_stubs()
    ls_mod, nm_mod, model_mod = _import_siren()
    out = {}
    gen_linear_sine(out, ls_mod)
    gen_model(out, nm_mod)
    gen_siren(out, model_mod)
    np.savez_compressed(os.path.join(OUT, "siren.npz"), **out)
    print("siren.npz", os.path.getsize(os.path.join(OUT, "siren.npz")), "bytes")
    for k in sorted(out):
        if k.startswith("dev.") and ".grad." not in k:
            print(k, out[k])
    worst = np.array([out[k][:2] / max(out[k][2], 1e-30) for k in out if k.startswith("dev.model.grad.")]).max(axis=0)
    print("dev.model.grad.* worst, relative to each tensor's maximum:", worst)
