"""2d-ingp (the Gigapixel image fit): a 2-D hash grid and a small ReLU MLP on gfx950 kernels.

Mirrors 2d-ingp/model.py name for name — same constructor arguments, submodule layout and parameter
creation order, so ``th.manual_seed`` gives the reference's initial values and state_dicts
interchange (``position_encoder.encodings.{l}.table``, ``net.{i}.weight`` / ``net.weight``):

* ``INGPTable(resolution, table_size, n_features, pi1, pi2)`` (model.py:13-86) — one level;
  ``bijective`` when ``table_size >= (resolution + 1)**2``; ``table`` of (r+1)^2 or table_size rows
  initialised ``(th.rand(rows, F) * 2 - 1) * 10**-4``; ``forward(x [N, 2])``.
* ``INGPEncoding(resolution_max, resolution_min, table_size, n_features, n_levels, pi1=1,
  pi2=2654435761)`` (model.py:90-115) — ``output_dim``, ``b``, ``resolution = th.floor(resolution_min *
  b ** th.arange(n_levels))`` in the reference's fp32 tensor arithmetic (2047, not 2048, at the top of
  main.py's schedule) and the ``encodings`` ModuleList.  The level Parameters are views of one packed
  buffer (the code of ``model_ingp.INGPEncoding``), so one ``nerf_hashgrid2d_fwd`` launch reads every
  level; the table gradient is the deterministic fixed-point ``nerf_hashgrid2d_bwd``.  Positions
  receive no gradient (the reference's are data): a position tensor that requires grad raises
  ``ValueError``.  ``last_status`` holds the device status word of the last forward: bit 0 set when
  a point outside [0, 1)^2 had a bijective-level corner dropped (the domain rule).
* ``Gigapixel(n_hidden, hidden_dim, position_encoder)`` (model.py:118-176) — ``net`` = Linear(enc, 3)
  when ``n_hidden == 0``, else the reference's Sequential with the same indices; ``forward(pos) ->
  sigmoid(net(enc(pos)))`` as one ``MLPFunction`` node with ReLU epilogues reading the encoding
  buffer; the sigmoid is a torch op, as in ``Nerf2d``.  ``training_step`` / ``validation_step`` /
  ``test_step`` return the MSE without Lightning logging; ``configure_optimizers`` as the reference
  (``FusedAdam`` on the GPU).
* ``pixel_centres(resolution, device)`` — the data module's coordinates; ``Gigapixel.render`` — the
  image logger's picture.
"""
from __future__ import annotations

import math

import torch as th
import torch.nn as nn

from . import kernels as K
from . import model_ingp as _ingp3
from .mlp import LayerPlan, MLPFunction, MLPPlan, Source


def _params(levels, table_size, n_features, resolutions, pi1, pi2):
    return K.make_hashgrid_params(levels, table_size, n_features, resolutions, 0, primes=(pi1, pi2, 0),
                                  normalize=False)


class _HashGrid2dFn(th.autograd.Function):
    """Features of every level in one launch; each level's table gradient is a view of one packed
    fixed-point gradient."""

    @staticmethod
    def forward(ctx, params, packed, rows, out_cols, x, status, *tables):
        n = x.shape[0]
        used = params.levels * params.features
        out = th.empty(n, out_cols, device=packed.device, dtype=th.float32)
        if out_cols > used:
            out[:, used:].zero_()
        K.hashgrid2d_fwd(params, packed, out, x, n, status)
        ctx.params, ctx.rows, ctx.shape = params, rows, packed.shape
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        grads = [None] * len(ctx.rows)
        if g is not None and any(ctx.needs_input_grad[6:]):
            gp = th.empty(ctx.shape, device=g.device, dtype=th.float32)
            ws = th.empty((K.hashgrid2d_workspace_bytes(ctx.params) + 7) // 8, dtype=th.int64, device=g.device)
            K.hashgrid2d_bwd(ctx.params, g.contiguous(), gp, ws, x, x.shape[0])
            off = 0
            for l, r in enumerate(ctx.rows):
                grads[l] = gp[off:off + r]
                off += r
        return (None,) * 6 + tuple(grads)


def _points(x: th.Tensor) -> th.Tensor:
    if not isinstance(x, th.Tensor) or x.dim() != 2 or x.shape[1] != 2:
        raise ValueError(f"x must be [N, 2] (got {tuple(getattr(x, 'shape', ()))})")
    if x.requires_grad:
        raise ValueError("the 2-D hash grid gives positions no gradient (the reference's are data): detach x")
    K._require_cuda_f32("x", x)
    return x.contiguous()


class INGPTable(nn.Module):
    def __init__(self, resolution, table_size, n_features, pi1, pi2):
        super().__init__()
        self.resolution = resolution
        self.table_size = table_size
        self.n_features = n_features
        self.pi1 = pi1
        self.pi2 = pi2
        self.bijective = table_size >= (resolution + 1) ** 2
        rows = (resolution + 1) ** 2 if self.bijective else table_size
        self.table = nn.Parameter((th.rand((rows, n_features)) * 2 - 1) * 10 ** (-4))
        self.last_status: th.Tensor | None = None

    def forward(self, x: th.Tensor) -> th.Tensor:
        """Features [N, n_features] of points x [N, 2] in [0, 1)."""
        x = _points(x)
        table = self.table
        if not table.is_contiguous():
            raise ValueError("INGPTable.table must be contiguous")
        self.last_status = th.zeros(1, dtype=th.int32, device=x.device)
        params = _params(1, self.table_size, self.n_features, [int(self.resolution)], self.pi1, self.pi2)
        return _HashGrid2dFn.apply(params, table, [table.shape[0]], self.n_features, x, self.last_status, table)


class INGPEncoding(nn.Module):
    def __init__(self, resolution_max, resolution_min, table_size, n_features, n_levels, pi1=1, pi2=2654435761):
        super().__init__()
        self.output_dim = n_features * n_levels
        self.resolution_max = resolution_max
        self.resolution_min = resolution_min
        self.table_size = table_size
        self.n_features = n_features
        self.n_levels = n_levels
        self.pi1, self.pi2 = pi1, pi2
        self.b = 1 if n_levels == 1 else math.exp((math.log(resolution_max) - math.log(resolution_min)) / (n_levels - 1))
        self.resolution = th.floor(resolution_min * self.b ** th.arange(n_levels))
        self.encodings = nn.ModuleList([INGPTable(int(r), table_size, n_features, pi1, pi2) for r in self.resolution])
        self.resolutions = [int(e.resolution) for e in self.encodings]
        self._rows = [e.table.shape[0] for e in self.encodings]
        self._packed_table = None
        self.last_status: th.Tensor | None = None
        self._pack()

    # the level Parameters as views of one buffer: model_ingp.INGPEncoding's own functions (they use
    # only encodings, _rows, n_features and _packed_table), borrowed so the 3-D class stays as it is
    _aliased = _ingp3.INGPEncoding._aliased
    _pack = _ingp3.INGPEncoding._pack
    packed_table = _ingp3.INGPEncoding.packed_table

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._pack()
        return out

    @property
    def padded_dim(self) -> int:
        return K.pad32(self.output_dim)

    def _hash_params(self):
        return _params(self.n_levels, self.table_size, self.n_features, self.resolutions, self.pi1, self.pi2)

    def encode_padded(self, x: th.Tensor) -> th.Tensor:
        """[N, pad32(output_dim)] features (pad columns zero): the buffer the MLP's first layer reads."""
        x = _points(x)
        packed = self._pack()
        self.last_status = th.zeros(1, dtype=th.int32, device=x.device)
        return _HashGrid2dFn.apply(self._hash_params(), packed, self._rows, self.padded_dim, x, self.last_status,
                                   *[e.table for e in self.encodings])

    def forward(self, x: th.Tensor) -> th.Tensor:
        return self.encode_padded(x)[:, :self.output_dim]


def pixel_centres(resolution: int, device=None) -> th.Tensor:
    """[resolution^2, 2] pixel-centre coordinates of the reference's data module, bitwise: the ``ij``
    meshgrid of ``arange(resolution).float() / resolution`` flattened, then ``+= 1 / 2 / resolution``."""
    axis = th.arange(resolution, device=device).float() / resolution
    pos = th.stack(th.meshgrid(axis, axis, indexing="ij"), dim=-1).reshape(-1, 2)
    pos += 1 / 2 / resolution
    return pos


class Gigapixel(nn.Module):
    def __init__(self, n_hidden: int, hidden_dim: int, position_encoder: INGPEncoding):
        super().__init__()
        self.n_hidden = n_hidden
        self.hidden_dim = hidden_dim
        self.position_encoder = position_encoder
        if self.n_hidden == 0:
            self.net = nn.Linear(self.position_encoder.output_dim, 3)
        else:
            layer1 = nn.Linear(self.position_encoder.output_dim, hidden_dim)
            layer2 = nn.Linear(hidden_dim, 3)
            intermediate_layers = []
            for _ in range(self.n_hidden - 1):
                intermediate_layers += [nn.ReLU(True), nn.Linear(hidden_dim, hidden_dim)]
            self.net = nn.Sequential(layer1, *intermediate_layers, nn.ReLU(True), layer2)
        self.sigmoid = nn.Sigmoid()
        self._plan: MLPPlan | None = None

    def _get_plan(self) -> MLPPlan:
        if self._plan is None:
            d = self.position_encoder.output_dim
            enc = Source("pos", d, K.pad32(d))
            if self.n_hidden == 0:
                layers = [LayerPlan(self.net, [enc], False)]
            else:
                h = self.hidden_dim
                linears = [m for m in self.net if isinstance(m, nn.Linear)]
                layers = [LayerPlan(linears[0], [enc], True)]
                for i, lin in enumerate(linears[1:], 1):
                    layers.append(LayerPlan(lin, [Source("act", h, K.pad32(h), i - 1)], i < len(linears) - 1))
            self._plan = MLPPlan(layers, [len(layers) - 1])
        return self._plan

    def forward(self, pos: th.Tensor) -> th.Tensor:
        plan = self._get_plan()
        enc = self.position_encoder.encode_padded(pos)
        (head,) = MLPFunction.apply(plan, pos.shape[0], enc, None, 1, *plan.params())
        return th.sigmoid(head[:, :3])

    def step_helper(self, stage: str, batch, batch_idx: int = 0) -> th.Tensor:
        pos, rgb = batch
        return nn.functional.mse_loss(self(pos), rgb)

    def training_step(self, batch, batch_idx: int = 0) -> th.Tensor:
        return self.step_helper("train", batch, batch_idx)

    def validation_step(self, batch, batch_idx: int = 0) -> th.Tensor:
        return self.step_helper("val", batch, batch_idx)

    def test_step(self, batch, batch_idx: int = 0) -> th.Tensor:
        return self.step_helper("test", batch, batch_idx)

    def configure_optimizers(self):
        # model.py:164-176; on the GPU Adam's step is nerf_amd's fused launch
        from .optim import FusedAdam
        params = list(self.parameters())
        optimizer = (FusedAdam if all(p.is_cuda for p in params) else th.optim.Adam)(params, lr=1e-3)
        scheduler = th.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=0.5, patience=5)
        return {"optimizer": optimizer, "lr_scheduler": scheduler, "monitor": "train_loss"}

    def render(self, resolution: int, chunk: int = 2 ** 20) -> th.Tensor:
        """[resolution, resolution, 3]: the image logger's ``self(pos).view(W, H, 3).permute(1, 0, 2)``
        on the pixel centres, without autograd, ``chunk`` points at a time."""
        dev = next(self.parameters()).device
        pos = pixel_centres(resolution, dev)
        out = th.empty(pos.shape[0], 3, device=dev, dtype=th.float32)
        with th.no_grad():
            for i in range(0, pos.shape[0], chunk):
                out[i:i + chunk] = self(pos[i:i + chunk])
        return out.view(resolution, resolution, 3).permute(1, 0, 2)


__all__ = ["INGPTable", "INGPEncoding", "Gigapixel", "pixel_centres"]
