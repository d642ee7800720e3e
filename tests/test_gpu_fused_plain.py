"""The plain-layer loop of the fused field-MLP kernels (csrc/mlp_fused.hip: `epi_plain`, taken by
layers that are register-fed only, N a multiple of 32 and <= 256, dense rows, no column / second
output) against the same build's generic loop on the same layers (NERF_FUSED_GENERIC through
`mlp_fused.FORCE_GENERIC`): every layer output, ReLU mask row, dY row, encoding gradient and
parameter gradient must be bit-identical — the plain loop only drops stores that were addressed out
of range and tests that were constant for the layer.

One small field holds every kind of layer, lowered with the helpers tests/test_gpu_fused.py uses
(LayerPlan / MLPPlan / MLPFunction; the network of barf/model_interpolation_architecture.py:96-141
with other widths):

    0  encoding-fed first layer (pos 60 -> 256, ReLU)
    1  256 -> 256 ReLU            plain, 16 chunks
    2  256 -> 128 ReLU            plain, 8 chunks: only mask word 0
    3  128 -> 256 ReLU            (4 register-fed k-blocks: generic)
    4  256 -> 256 ReLU            plain
    5  256 -> 257, column output  the density + feature layer: 17 chunks, an odd count, the last alone
    6  [256 | dir 24] -> 128 ReLU (HBM-fed k-block: generic)
    7  128 -> 4 head              one chunk, an odd count

The input-gradient chain of this plan runs plain steps of 16 chunks (layers 4 and 1) and of 8 chunks
(layer 3, whose input is 128 wide) between generic ones (second outputs, HBM-fed gradient blocks).
The chain takes heads of at most 32 columns, so a head with three chunks (N = 48) is checked in the
forward only.  M: a full tile, a partial tile ending in a partial wave, several tiles ending partial.

Tolerances against the layer-by-layer path are the existing ones of tests/test_gpu_fused.py: layer
outputs within 1e-4 of the layer's max |value|; every gradient's error against fp64 (relative to the
tensor's max |gradient|) no worse than the layer-by-layer backward's + 1e-2.  Those tests also cap
the error against fp64 at 5e-2, a statement about batches of 4096 and more samples that the
layer-by-layer path itself does not meet here: with a few hundred samples one ReLU unit whose
pre-activation lies within 2^-17 of zero, dead in fp64 and alive in split precision, moves a bias
gradient by several percent of its scale (measured at M = 309, layer 0's bias: layer-by-layer 6.16e-2,
fused 6.28e-2; every other tensor and size <= 1.2e-2), so the cap is not asserted.  For the same
reason the two split-precision paths, which sum in different orders, can disagree on the state of a
ReLU unit whose pre-activation is within their rounding of zero (measured at M = 309: layer 3, sample
31, unit 124: 0.0 layer by layer, 1.0e-7 fused).  ReLU' is discontinuous there: that unit's row of
the layer's weight and bias gradient then differs by the whole contribution of that sample (2.0e-2
of the tensor's scale among 309 samples; every other row <= 7e-6, earlier layers <= 3e-3).  The test
requires every such disagreement to lie inside the forward tolerance of zero on both paths and leaves
those units' rows of that layer's gradients out of the comparison with fp64; nothing else.  In "medium" (one
bf16 pass) the layer-by-layer comparison is the one of tests/test_gpu_medium.py; here the plain loop
must equal the generic one bit for bit.  Pad columns and guard bytes: the checker of
tests/test_gpu_guard_bands.py."""
import pytest
import torch
from torch import nn

import test_gpu_guard_bands as GB

pytestmark = pytest.mark.gpu
DEV = "cuda"
MS = [128, 309, 1061]


def _plan(head_n=4, dtype=torch.float32):
    from nerf_amd import kernels as K
    from nerf_amd.mlp import LayerPlan, MLPPlan, Source
    torch.manual_seed(3)
    dims = [(60, 256), (256, 256), (256, 128), (128, 256), (256, 256), (256, 257), (256 + 24, 128), (128, head_n)]
    lins = nn.ModuleList([nn.Linear(i, o) for i, o in dims]).to(DEV).to(dtype)
    pos = Source("pos", 60, K.pad32(60))
    dirs = Source("dir", 24, K.pad32(24))
    layers = [LayerPlan(lins[0], [pos], True)]
    for l in range(1, 8):
        k = 128 if dims[l][0] == 128 else 256
        srcs = [Source("act", k, K.pad32(k), l - 1)] + ([dirs] if l == 6 else [])
        layers.append(LayerPlan(lins[l], srcs, l not in (5, 7)))
    return MLPPlan(layers, [5, 7], [(5, 256)]), lins


def _inputs(M, pos_grad):
    g = torch.Generator(device=DEV).manual_seed(21 + M)
    pos = torch.zeros(M, 64, device=DEV)
    pos[:, :60] = torch.rand(M, 60, device=DEV, generator=g) * 2 - 1
    dirs = torch.zeros(M, 32, device=DEV)
    dirs[:, :24] = torch.rand(M, 24, device=DEV, generator=g) * 2 - 1
    w_head = torch.randn(M, 4, device=DEV, generator=g)
    w_sig = torch.randn(M, device=DEV, generator=g)
    return pos.requires_grad_(pos_grad), dirs, w_head, w_sig


def _run(M, mode, backward, head_n=4, monkeypatch=None):
    """mode: "layerwise" | "generic" | "plain".  Returns the captured tensors of one step."""
    from nerf_amd import mlp, mlp_fused
    from nerf_amd.mlp import MLPFunction
    plan, lins = _plan(head_n)
    pos, dirs, w_head, w_sig = _inputs(M, backward)
    rec = {}
    orig = mlp_fused.FusedInputGrad.run

    def chain_run(self, M_, g_head, dY, masks, g_cols=None, x_out=None, **kw):
        r = orig(self, M_, g_head, dY, masks, g_cols, x_out, **kw)
        rec["dY"] = [None if t is None else t.clone() for t in dY]
        rec["x_out"] = {l: t.clone() for l, t in (x_out or {}).items()}
        return r

    plan.to_device(torch.device(DEV))
    assert mlp_fused.eligible(plan, M) and (not backward or mlp_fused.dgrad_eligible(plan, M))
    saved = mlp_fused.ENABLED, mlp_fused.FORCE_GENERIC
    mlp_fused.ENABLED = mode != "layerwise"
    mlp_fused.FORCE_GENERIC = mode == "generic"
    mlp_fused.FusedInputGrad.run = chain_run
    mlp.CAPTURE = []
    runs = mlp_fused.FusedInputGrad.runs
    try:
        outs = MLPFunction.apply(plan, M, pos, dirs, 1, *plan.params())
        if backward:
            ((outs[1][:, :4] * w_head).sum() + (outs[2] * w_sig).sum()).backward()
        torch.cuda.synchronize()
        acts, masks = mlp.CAPTURE[0]
    finally:
        mlp_fused.ENABLED, mlp_fused.FORCE_GENERIC = saved
        mlp_fused.FusedInputGrad.run = orig
        mlp.CAPTURE = None
    if backward:
        assert (mlp_fused.FusedInputGrad.runs > runs) == (mode != "layerwise")
        rec["grads"] = {n: p.grad.detach().clone() for n, p in lins.named_parameters()}
        rec["pos"] = pos.grad.detach().clone()
    rec.update(acts=[a.clone() for a in acts], masks=[None if m is None else m.clone() for m in masks],
               outs=[o.detach().clone() for o in outs], plan=plan)
    return rec


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), what


def _assert_identical(p, g, backward):
    for l, (a, b) in enumerate(zip(p["acts"], g["acts"])):
        _same(a, b, f"layer {l} output")
    for l, (a, b) in enumerate(zip(p["masks"], g["masks"])):
        _same(a, b, f"layer {l} mask row")
    for i, (a, b) in enumerate(zip(p["outs"], g["outs"])):
        _same(a, b, f"output {i}")
    if backward:
        assert len(p["dY"]) == len(g["dY"]) and any(t is not None for t in p["dY"])
        for l, (a, b) in enumerate(zip(p["dY"], g["dY"])):
            _same(a, b, f"dY of layer {l}")
        assert p["x_out"].keys() == g["x_out"].keys() and p["x_out"]
        for l in p["x_out"]:
            _same(p["x_out"][l], g["x_out"][l], f"encoding gradient of layer {l}")
        _same(p["pos"], g["pos"], "position-encoding gradient")
        for n in p["grads"]:
            _same(p["grads"][n], g["grads"][n], f"gradient of {n}")


def _fp64_grads(M):
    plan, lins = _plan(dtype=torch.float64)
    pos, dirs, w_head, w_sig = _inputs(M, False)
    p64 = pos.double().requires_grad_(True)
    acts = []
    for lp in plan.layers:
        parts = [(acts[s.layer] if s.kind == "act" else (p64 if s.kind == "pos" else dirs.double()))[:, :s.k_valid]
                 for s in lp.sources]
        y = nn.functional.linear(torch.cat(parts, 1), lp.module.weight, lp.module.bias)
        acts.append(torch.relu(y) if lp.relu else y)
    ((acts[7][:, :4] * w_head.double()).sum() + (acts[5][:, 256] * w_sig.double()).sum()).backward()
    out = {n: p.grad.detach() for n, p in lins.named_parameters()}
    out["pos"] = p64.grad.detach()
    return out


@pytest.fixture
def precision(request):
    import nerf_amd
    nerf_amd._lib.load()
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(request.param)
    yield request.param
    torch.set_float32_matmul_precision(old)


@pytest.mark.parametrize("precision", ["high", "medium"], indirect=True)
@pytest.mark.parametrize("M", MS)
def test_plain_loop_is_bit_identical_to_generic(M, precision):
    """Forward and backward: plain == generic bit for bit; in "high" both within the existing
    tolerance of the layer-by-layer path (outputs) and of fp64 (gradients)."""
    plain = _run(M, "plain", True)
    generic = _run(M, "generic", True)
    _assert_identical(plain, generic, True)
    plan = plain["plan"]
    # pad columns of the fused outputs are zero (the 257-wide layer's row stride is 260)
    for l, a in enumerate(plain["acts"]):
        n = plan.layers[l].N
        if a.shape[1] > n:
            assert (a[:, n:] == 0).all(), l
    if precision != "high":
        return
    ref = _run(M, "layerwise", True)
    for l, (x, y) in enumerate(zip(ref["acts"], plain["acts"])):
        n = plan.layers[l].N
        scale = max(1.0, x[:, :n].abs().max().item())
        err = (x[:, :n] - y[:, :n]).abs().max().item()
        print(f"layer {l}: max |fused - layerwise| = {err:.3e} (scale {scale:.3e})")
        assert err <= 1e-4 * scale, (l, err, scale)
    # units whose ReLU state differs between the two paths: only inside the forward tolerance of zero
    flipped = {}
    for l, lp in enumerate(plan.layers):
        if lp.relu:
            x, y = ref["acts"][l][:, :lp.N], plain["acts"][l][:, :lp.N]
            d = (x > 0) != (y > 0)
            assert (torch.maximum(x.abs(), y.abs())[d] <= 1e-4 * max(1.0, x.abs().max().item())).all(), l
            flipped[l] = d.any(0)
            print(f"layer {l}: {int(d.sum())} ReLU states differ between the paths (units {d.any(0).nonzero().flatten().tolist()})")
    r64 = _fp64_grads(M)
    for n, r in r64.items():
        scale = max(r.abs().max().item(), 1e-12)
        lay = ref["pos"] if n == "pos" else ref["grads"][n]
        fus = plain["pos"] if n == "pos" else plain["grads"][n]
        assert lay.shape == r.shape == fus.shape, n
        keep = torch.ones(r.shape[0], dtype=torch.bool, device=r.device)
        if n != "pos" and int(n.split(".")[0]) in flipped:
            keep = ~flipped[int(n.split(".")[0])]
        e_layer = (lay.double() - r)[keep].abs().max().item() / scale
        e_fused = (fus.double() - r)[keep].abs().max().item() / scale
        print(f"{n}: fused {e_fused:.3e} layerwise {e_layer:.3e} ({int((~keep).sum())} rows of units with differing ReLU state left out)")
        assert e_fused <= e_layer + 1e-2, (n, e_fused, e_layer)


@pytest.mark.parametrize("precision", ["high", "medium"], indirect=True)
def test_plain_forward_with_three_chunk_head(precision):
    """A head of N = 48 (three chunks: an odd count) after the plain layers, forward only (the chain
    takes heads of at most 32 columns)."""
    M = 309
    plain = _run(M, "plain", False, head_n=48)
    generic = _run(M, "generic", False, head_n=48)
    _assert_identical(plain, generic, False)
    if precision == "high":
        ref = _run(M, "layerwise", False, head_n=48)
        for l, (x, y) in enumerate(zip(ref["acts"], plain["acts"])):
            n = plain["plan"].layers[l].N
            scale = max(1.0, x[:, :n].abs().max().item())
            assert (x[:, :n] - y[:, :n]).abs().max().item() <= 1e-4 * scale, l


@pytest.mark.parametrize("precision", ["high", "medium"], indirect=True)
@pytest.mark.parametrize("M", [309, 1061])
def test_plain_loop_leaves_guard_bytes_and_pad_columns(M, precision, monkeypatch):
    """One forward + backward with every device buffer of the step between sentinel-filled guard
    regions: no byte outside a buffer changes, pad columns hold the sentinel or zero."""
    import importlib
    import pkgutil

    import nerf_amd
    for m in pkgutil.iter_modules(nerf_amd.__path__):
        if not m.name.startswith("lib"):
            importlib.import_module("nerf_amd." + m.name)
    lib = nerf_amd._lib.load()
    gt = GB._install(monkeypatch)
    regions, calls, extra = GB._record_fused_outputs(monkeypatch, lib)
    rec = _run(M, "plain", True)
    assert calls.get("nerf_mlp_fused_run", 0) >= 2, calls
    assert len(gt.allocs) > 10
    # dY of the 257-wide layer: the chain writes its 256 register-fed columns; columns 256..259 are
    # the backward's own (mlp.py zeroes them and adds the column output's gradient at 256), declared
    # here as the checker's "columns another output of the step writes"
    ld5 = rec["plan"].layers[5].out_ld
    mine = [(ptr + 4 * ncols, ld) for _, _, ptr, _, ld, ncols in regions if ld == ld5 and ncols == 256]
    assert len(mine) == 1 and ld5 == 260
    assert GB._check(gt, regions, list(extra) + mine) > 1
