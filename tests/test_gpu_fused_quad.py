"""Hidden activations saved quad-split by the fused forward (mlp.SAVE_SPLIT, NERF_FUSED_SPLIT_OUT;
include/nerf_amd.h) and read back by the weight-gradient tile kernel: a training step with the
switch on computes bit for bit what it computes with the switch off — every exposed output and
every parameter gradient torch.equal — on the n2v and barf NerfModels of tests/test_gpu_fused.py
and the mip plan (skip layer, 257-row layer), at sizes with a partial tile, several tiles, and whole
rays of 64 samples (the per-ray weight-gradient route).  The stored words of every selected layer
are the host packing (kernels.quad_split_pack) of the fp32 activation the other run stored, pad
columns included; the other layers' buffers are equal.  Also: the launched flags against the
selection rule, the CAPTURE and dgrad_eligible gates, and the layer-by-layer input gradients after
a quad-split forward (a gradient on the exposed feature output), which take the ReLU bits instead
of the activation."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(3 * 64 + 5, 1), (1000, 1), (128 * 3, 64)]


@pytest.fixture(scope="module", autouse=True)
def _precision():
    import nerf_amd
    nerf_amd._lib.load()
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("high")
    yield
    torch.set_float32_matmul_precision(prev)


def _model(name):
    from nerf_amd import BarfPositionalEncoding, FourierFeatures, NerfModel
    from nerf_amd.positional_encodings import IntegratedBarfFourierFeatures
    torch.manual_seed(0)
    if name == "n2v":
        return NerfModel(4, 256, True, True, 2, FourierFeatures(10, 2 * math.pi), FourierFeatures(4, 1.0))
    if name == "barf":
        return NerfModel(4, 256, True, False, 2, BarfPositionalEncoding(10, 10.0, 0, 1, True, 1.0),
                         BarfPositionalEncoding(4, 4.0, 0, 1, True, 1.0))
    ipe = IntegratedBarfFourierFeatures(10, 10, 1.28, 6.4, True, 1.0, True)
    ipe.pixel_width_sigma = 0.0
    return NerfModel(4, 256, True, False, 2, ipe, BarfPositionalEncoding(4, 4, 1.28, 6.4, True, 1.0))


def _inputs(model, M, rd, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pd, dd = model.position_encoder.output_dim, model.direction_encoder.output_dim
    pos = torch.zeros(M, (pd + 31) // 32 * 32, device=DEV)
    pos[:, :pd] = torch.rand(M, pd, device=DEV, generator=g) * 2 - 1
    nd = (M + rd - 1) // rd
    dirs = torch.zeros(nd, (dd + 31) // 32 * 32, device=DEV)
    dirs[:, :dd] = torch.rand(nd, dd, device=DEV, generator=g) * 2 - 1
    return pos, dirs, g


def _step(name, M, rd, split, feature_grad=False, seed=5):
    """One forward + backward: (outputs, saved activations, parameter gradients, launched flags, plan)."""
    from nerf_amd import mlp
    from nerf_amd.mlp import MLPFunction
    model = _model(name).to(DEV)
    plan = model._get_plan()
    pos, dirs, g = _inputs(model, M, rd, seed)
    saved = mlp.SAVE_SPLIT
    mlp.SAVE_SPLIT = split
    try:
        outs = MLPFunction.apply(plan, M, pos, dirs, rd, *plan.params())
        L = len(plan.layers)
        acts = [t.clone() for t in outs[0].grad_fn.saved_tensors[2:2 + L]]
        loss = 0.0
        for i, o in enumerate(outs):
            if i == 0 and not feature_grad:
                continue                    # the exposed feature layer: no gradient, the chain runs
            o2 = o.reshape(M, -1)
            if i < len(plan.outputs):
                o2 = o2[:, :plan.layers[plan.outputs[i]].N]        # (padding columns: unspecified)
            loss = loss + (o2 * torch.randn(o2.shape, device=DEV, generator=g)).sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        mlp.SAVE_SPLIT = saved
    flags = next(iter(plan.fused.values())).last_flags
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    return [o.detach().clone() for o in outs], acts, grads, flags, plan


def _split_of(flags):
    return frozenset(l for l in range(16) if (flags >> (8 + l)) & 1)


@pytest.mark.parametrize("name", ["n2v", "barf", "mip"])
@pytest.mark.parametrize("M,rd", SIZES)
def test_training_step_is_bit_identical_with_quad_split_activations(name, M, rd, monkeypatch):
    from nerf_amd import kernels as K, mlp, mlp_fused
    o0, a0, g0, f0, plan = _step(name, M, rd, False)
    o1, a1, g1, f1, _ = _step(name, M, rd, True)
    assert _split_of(f0) == frozenset()
    monkeypatch.setattr(mlp, "SAVE_SPLIT", True)
    want = mlp.split_layers(plan, M, rd)
    assert _split_of(f1) == want and want
    if name == "mip":
        assert want == frozenset(range(8))
    assert len(o0) == len(o1)
    for x, y in zip(o0, o1):
        assert torch.equal(x, y)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    for l, (x, y) in enumerate(zip(a0, a1)):
        nz = x[x != 0].abs()
        assert torch.isfinite(x).all() and (nz.numel() == 0 or nz.min() >= 2.0 ** -120), l   # (else: another seed)
        if l in want:
            assert torch.equal(y.view(torch.int32), K.quad_split_pack(x).view(torch.int32)), l
        else:
            assert torch.equal(x, y), l


def test_no_layer_is_split_under_capture_or_without_the_chain(monkeypatch):
    from nerf_amd import mlp, mlp_fused
    from nerf_amd.mlp import MLPFunction
    M, rd = 1000, 1
    model = _model("mip").to(DEV)
    plan = model._get_plan()
    pos, dirs, _ = _inputs(model, M, rd, 5)
    monkeypatch.setattr(mlp, "SAVE_SPLIT", True)
    mlp.CAPTURE = []
    try:
        MLPFunction.apply(plan, M, pos, dirs, rd, *plan.params())
        acts, _ = mlp.CAPTURE[0]
    finally:
        mlp.CAPTURE = None
    fused = next(iter(plan.fused.values()))
    assert _split_of(fused.last_flags) == frozenset()
    MLPFunction.apply(plan, M, pos, dirs, rd, *plan.params())
    assert _split_of(fused.last_flags) == frozenset(range(8))
    monkeypatch.setattr(mlp_fused, "dgrad_eligible", lambda plan, M: False)
    MLPFunction.apply(plan, M, pos, dirs, rd, *plan.params())
    assert _split_of(fused.last_flags) == frozenset()
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["n2v", "mip"])
def test_layerwise_input_gradients_after_a_quad_split_forward(name):
    """A gradient on the exposed feature output keeps the backward off the chain: the
    layer-by-layer GEMMs take the ReLU mask from the stored bits, never from the split words."""
    from nerf_amd import mlp_fused
    M, rd = 1000, 1
    runs = mlp_fused.FusedInputGrad.runs
    o0, _, g0, _, _ = _step(name, M, rd, False, feature_grad=True)
    o1, _, g1, f1, _ = _step(name, M, rd, True, feature_grad=True)
    assert mlp_fused.FusedInputGrad.runs == runs and _split_of(f1)
    for x, y in zip(o0, o1):
        assert torch.equal(x, y)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_split_flag_argument_errors():
    from nerf_amd import _lib, mlp
    from nerf_amd.mlp import MLPFunction
    M = 256
    model = _model("barf").to(DEV)
    plan = model._get_plan()
    pos, dirs, _ = _inputs(model, M, 1, 5)
    MLPFunction.apply(plan, M, pos, dirs, 1, *plan.params())
    fused = next(iter(plan.fused.values()))
    L = len(plan.layers)

    def run(split_out, passes=3):
        acts = [torch.empty(M, lp.out_ld, device=DEV) for lp in plan.layers]
        masks = [torch.empty(M, 32, device=DEV, dtype=torch.uint8) if lp.relu and lp.N <= 256 else None
                 for lp in plan.layers]
        cols = {li: torch.empty(M, device=DEV) for li, _ in plan.column_outputs}
        fused.run(M, pos, dirs, 1, acts, masks, cols, passes=passes, split_out=split_out)

    run([0, 3])
    for bad in ([L - 1], [9]):                # the last layer; the 257-wide layer with the column output
        with pytest.raises(RuntimeError, match="status -1"):
            run(bad)
    with pytest.raises(RuntimeError, match="status -1"):
        run([0], passes=1)                    # NERF_FUSED_BF16
    torch.cuda.synchronize()
