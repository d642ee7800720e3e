"""Golden data of the 2-D hash-grid image fit, produced by the reference's own module
(2d-ingp/model.py: INGPTable, INGPEncoding, Gigapixel), imported from its directory with import
stubs for the absent pytorch_lightning and its data_loader, and run eagerly on the CPU.  Writes
ingp2d.npz next to this file.  Usage:

    NERF_REFERENCE=/path/to/nerf-experiments python tests/golden/make_golden_ingp2d.py

Two configurations, each built under ``th.manual_seed(0)`` (encoder first, then the model):
  A  INGPEncoding(64, 4, 2**8, 2, 5)   resolutions 4, 8, 16, 32, 64 (4, 8 bijective), Gigapixel(2, 64, enc)
  B  INGPEncoding(100, 3, 1000, 4, 4)  resolutions 3, 9, 31, 100 (3, 9 bijective; a table size that
                                       is no power of two), Gigapixel(0, 64, enc)
Per configuration (keys ``A.*`` / ``B.*``): state_dict key names and init checksums
(``sdsum.*``: sum, sum |.|), then the tables multiplied by 1e3 (so that features and their gradients
are not lost below the biases) and from that state: the state_dict (``sd.*``), resolutions and
bijective flags, the features of ``x``, rgb, the MSE loss against ``y``, every parameter's gradient
(``grad.*``) and the parameters after three torch-Adam steps at lr 1e-3 (``adam3.*``).
Shared: ``x`` [503, 2] = 300 pixel centres of a 16 x 16 grid (drawn with replacement), 200 uniform
points of [0, 1)^2 and (0, 0), (0.999999, 0.5), (1 - 2^-24, 1 - 2^-24); ``y`` [503, 3] uniform.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch as th

REF = os.environ.get("NERF_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def _import_model():
    pl = types.ModuleType("pytorch_lightning")

    class LightningModule(th.nn.Module):
        def log(self, *a, **k):
            pass

    pl.LightningModule = LightningModule
    dl = types.ModuleType("data_loader")
    dl.SingleImageDataModule = object
    saved = {n: sys.modules.get(n) for n in ("pytorch_lightning", "data_loader", "model")}
    sys.modules["pytorch_lightning"], sys.modules["data_loader"] = pl, dl
    sys.modules.pop("model", None)
    sys.path.insert(0, os.path.join(REF, "2d-ingp"))
    try:
        return importlib.import_module("model")
    finally:
        sys.path.pop(0)
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def f32(t):
    return t.detach().to(th.float32).numpy().copy()


def inputs():
    g = th.Generator().manual_seed(19)
    res = 16
    xi, yi = th.meshgrid(th.arange(res), th.arange(res), indexing="ij")
    centres = th.hstack((xi.flatten().float().unsqueeze(1) / res, yi.flatten().float().unsqueeze(1) / res))
    centres += 1 / 2 / res
    pick = th.randint(0, res * res, (300,), generator=g)
    edge = th.tensor([[0.0, 0.0], [0.999999, 0.5], [1 - 2.0 ** -24, 1 - 2.0 ** -24]])
    x = th.cat((centres[pick], th.rand(200, 2, generator=g), edge))
    y = th.rand(x.shape[0], 3, generator=g)
    return x, y


def config(out, M, tag, enc_args, n_hidden, x, y):
    th.manual_seed(0)
    enc = M.INGPEncoding(*enc_args)
    model = M.Gigapixel(n_hidden, 64, enc)
    out[f"{tag}.keys"] = np.array(list(model.state_dict().keys()))
    for k, v in model.state_dict().items():
        out[f"{tag}.sdsum.{k}"] = np.array([v.double().sum().item(), v.double().abs().sum().item()])
    with th.no_grad():
        for e in enc.encodings:
            e.table.mul_(1e3)
    for k, v in model.state_dict().items():
        out[f"{tag}.sd.{k}"] = f32(v)
    out[f"{tag}.res"] = np.array([int(e.resolution) for e in enc.encodings], dtype=np.int64)
    out[f"{tag}.bijective"] = np.array([bool(e.bijective) for e in enc.encodings])
    out[f"{tag}.features"] = f32(enc(x))
    rgb = model(x)
    loss = th.nn.functional.mse_loss(rgb, y)
    loss.backward()
    out[f"{tag}.rgb"], out[f"{tag}.loss"] = f32(rgb), f32(loss)
    for k, p in model.named_parameters():
        out[f"{tag}.grad.{k}"] = f32(p.grad)
    opt = th.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(3):
        opt.zero_grad()
        model.training_step((x, y), 0).backward()
        opt.step()
    for k, v in model.state_dict().items():
        out[f"{tag}.adam3.{k}"] = f32(v)


def main():
    M = _import_model()
    x, y = inputs()
    out = {"x": f32(x), "y": f32(y)}
    config(out, M, "A", (64, 4, 2 ** 8, 2, 5), 2, x, y)
    config(out, M, "B", (100, 3, 1000, 4, 4), 0, x, y)
    path = os.path.join(OUT, "ingp2d.npz")
    np.savez_compressed(path, **out)
    print("ingp2d.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
