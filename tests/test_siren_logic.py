"""SIREN networks without a GPU: construction and state-dict names against the reference's fixture
(tests/golden/siren.npz), the lowering of NerfModel to one MLPPlan, and the three new C entry
points (declared, bound, exported; argument validation before any launch)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import _siren_ref as R

NEW_SYMBOLS = ["nerf_sine_act_fwd", "nerf_sine_act_bwd", "nerf_linear_sine_x3"]


def _digest_close(t, want, what):
    np.testing.assert_allclose(np.array(R.digest(t)), want, rtol=1e-12, atol=1e-12, err_msg=what)


def test_model_construction_matches_reference_state(golden):
    """th.manual_seed(0) construction of NerfModel(32): the reference's key names, shapes and the
    (sum, abs-sum) of every parameter and buffer."""
    from nerf_amd import model_siren
    g = golden("siren")
    torch.manual_seed(0)
    m = model_siren.NerfModel(32)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["model.keys"]]
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in g["model.params"]]
    assert sum(p.numel() for p in m.parameters()) == 530_695
    for (k, v), shape in zip(sd.items(), g["model.shapes"]):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]], k
        _digest_close(v, g[f"model.sd.{k}"], k)


@pytest.mark.parametrize("case", R.LS_CASES, ids=[c[0] for c in R.LS_CASES])
def test_linear_sine_construction_and_recipes(golden, case):
    """LinearSine's RNG stream (uniform_ then the width, first layer or not) and the unstored
    inputs' recipes against their digests."""
    from nerf_amd import LinearSine
    g = golden("siren")
    key, k, n, first = case
    torch.manual_seed(0)
    m = LinearSine(k, n, scale=R.linear_sine_scale(key), first_layer=first)
    assert list(m.state_dict().keys()) == ["scale", "linear.weight", "linear.bias"]
    _digest_close(m.linear.weight, g[f"{key}.sd.weight"], "weight")
    _digest_close(m.linear.bias, g[f"{key}.sd.bias"], "bias")
    _digest_close(m.scale, g[f"{key}.sd.scale"], "scale")
    _digest_close(R.linear_sine_input(key, k), g[f"{key}.x.digest"], "x")
    _digest_close(R.upstream(n), g[f"{key}.gy.digest"], "gy")
    if f"{key}.x" in g:
        assert np.array_equal(R.linear_sine_input(key, k).numpy(), g[f"{key}.x"])


def test_linear_sine_constructor_checks():
    from nerf_amd import LinearSine
    assert LinearSine(4, 8, scale=2).scale.tolist() == [2.0] * 4        # an int scale is a float one
    with pytest.raises(AssertionError):
        LinearSine(4, 8, scale=0.0)
    with pytest.raises(AssertionError):
        LinearSine(4, 8, scale=torch.ones(3))
    with pytest.raises(AssertionError):
        LinearSine(4, 8, scale=torch.tensor([1.0, 1.0, -1.0, 1.0]))
    with pytest.raises(TypeError):
        LinearSine(4, 8, scale="1")


def test_load_reference_shaped_state_dict(golden):
    """A state dict with the reference's keys and shapes loads (strict), into NerfModel and into
    both networks of NerfSiren."""
    from nerf_amd import NerfSiren, model_siren
    g = golden("siren")
    ref = {str(k): torch.full([int(s) for s in shape if s > 0], 0.25)
           for k, shape in zip(g["model.keys"], g["model.shapes"])}
    m = model_siren.NerfModel(32)
    m.load_state_dict(ref, strict=True)
    assert all((v == 0.25).all() for v in m.state_dict().values())
    s = NerfSiren(1 / 3, 1.0, 32, 16)
    assert isinstance(s.model_coarse, model_siren.NerfModel) and isinstance(s.model_fine, model_siren.NerfModel)
    both = {f"{net}.{k}": v for net in ("model_coarse", "model_fine") for k, v in ref.items()}
    assert list(s.state_dict().keys()) == list(both.keys())
    s.load_state_dict(both, strict=True)
    # a loaded input scale the lowering does not apply is refused, not silently ignored
    with pytest.raises(ValueError):
        m._get_plan()


def test_plan_lowering():
    """One plan of the network's 10 Linear layers in execution order; the skip layers read
    [z | pos] and [rgb_latent | dir] as two segments; base colour and density leave as [M] columns of
    the 260-wide layer; the sine layers keep their pre-activation and have no parameters."""
    from nerf_amd import mlp_fused, model_siren
    m = model_siren.NerfModel(32)
    plan = m._get_plan()
    linears = [x for x in m.modules() if isinstance(x, torch.nn.Linear)]
    assert len(linears) == 10 and [id(lp.module) for lp in plan.layers] == [id(x) for x in linears]
    assert [lp.sine for lp in plan.layers] == [True] * 7 + [False, True, False]
    assert all(lp.keeps_pre == lp.sine and lp.pact == () and not lp.relu and not lp.tanh for lp in plan.layers)
    src = [[(s.kind, s.k_valid, s.k_pad, s.layer) for s in lp.sources] for lp in plan.layers]
    assert src[0] == [("pos", 3, 32, -1)]
    assert src[4] == [("act", 256, 256, 3), ("pos", 3, 32, -1)]         # model_density_2: [z | pos]
    assert src[8] == [("act", 256, 256, 7), ("dir", 3, 32, -1)]         # model_color: [rgb_latent | dir]
    for i in (1, 2, 3, 5, 6, 7, 9):
        assert src[i] == [("act", 256, 256, i - 1)]
    assert plan.layers[7].module.out_features == 260
    assert plan.outputs == [9]
    assert plan.column_outputs == [(7, 256), (7, 257), (7, 258), (7, 259)]      # r, g, b, density
    assert plan.params() == [t for x in linears for t in (x.weight, x.bias)]
    # sole consumers: every sine layer's backward can ride its consumer's input-gradient GEMM
    assert [plan.contributors[i] for i in range(10)] == [1, 1, 1, 1, 1, 1, 1, 5, 1, 1]
    assert all(lp.bwd_epilogue_fits(256) for lp in plan.layers if lp.sine)
    for lp in plan.layers:
        lp.finalize("cpu")
        assert sorted(c for c in lp.col_map.tolist() if c >= 0) == list(range(lp.module.in_features))
    assert all(mlp_fused._layer_shape(plan, i) is None for i, lp in enumerate(plan.layers) if lp.sine)
    assert not mlp_fused.eligible(plan, 1 << 16)


def test_sine_is_exclusive():
    from nerf_amd.mlp import LayerPlan, Source
    lin = torch.nn.Linear(4, 8)
    src = [Source("pos", 4, 32)]
    assert LayerPlan(lin, src, False, sine=True).keeps_pre
    assert not LayerPlan(lin, src, False).keeps_pre
    for kw in (dict(relu=True), dict(relu=False, tanh=True),
               dict(relu=False, gauss=torch.nn.Parameter(torch.ones(8))),
               dict(relu=False, act=(2, (torch.nn.Parameter(torch.ones(8)),)))):
        relu = kw.pop("relu")
        with pytest.raises(ValueError):
            LayerPlan(lin, src, relu, sine=True, **kw)


def test_renderer_is_shared_with_naive_ingp():
    from nerf_amd import NaiveINGP, NerfSiren
    from nerf_amd.model_ingp import CoarseFineRenderer
    assert issubclass(NaiveINGP, CoarseFineRenderer) and issubclass(NerfSiren, CoarseFineRenderer)
    for name in ("_sample_t_coarse", "_sample_t_fine", "_compute_positions", "_render_rays", "_compute_color",
                 "forward", "training_loss"):
        assert getattr(NerfSiren, name) is getattr(NaiveINGP, name) is getattr(CoarseFineRenderer, name), name
    s = NerfSiren(1 / 3, 1.0, 32, 16, learning_rate=2e-4, learning_rate_decay=0.25, weight_decay=0.0)
    cfg = s.configure_optimizers()
    assert isinstance(cfg["optimizer"], torch.optim.Adam) and cfg["optimizer"].defaults["lr"] == 2e-4
    assert cfg["optimizer"].defaults["betas"] == (0.9, 0.999) and cfg["optimizer"].defaults["eps"] == 1e-8
    assert isinstance(cfg["lr_scheduler"], torch.optim.lr_scheduler.ExponentialLR) and cfg["lr_scheduler"].gamma == 0.25


def test_new_symbols_declared_bound_and_exported():
    import nerf_amd
    from nerf_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_amd.h")).read(), flags=re.S)
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported
    # the sine is no activation kind, and no ABI bump
    assert re.search(r"#define\s+NERF_ACT_GABOR\s+1\b", src) and re.search(r"#define\s+NERF_ACT_SARF\s+2\b", src)
    assert not re.search(r"#define\s+NERF_ACT_SIN", src)
    assert (_lib.NERF_ACT_GABOR, _lib.NERF_ACT_SARF) == (1, 2)
    assert lib.nerf_abi_version() == 10
    assert nerf_amd.LinearSine is nerf_amd.model_siren.LinearSine and nerf_amd.NerfSiren is nerf_amd.model_siren.NerfSiren
    assert nerf_amd.NerfModel is not nerf_amd.model_siren.NerfModel


def test_argument_validation_returns_status_without_launch():
    from nerf_amd import _lib
    lib = _lib.load()
    P = 256        # any non-null, 16-byte aligned address: nothing is dereferenced before the checks
    # ---- the sine did not become a kind
    assert lib.nerf_param_act_fwd(3, P, 16, P, P, 10, 16, P, 16, None) == -1
    assert lib.nerf_param_act_workspace(3, 1000, 64) == 0
    assert lib.nerf_linear_act_workspace(3, 1000, 64) == 0
    assert lib.nerf_linear_act_x3(3, None, 0, 10, P, 32, 8, None, P, 8, 0, P, P, P, 8, None, 0, None, None, 0, None, 0,
                                  None) == -1
    # ---- nerf_sine_act_fwd(z, ld_z, M, N, y, ld_y, stream)
    assert lib.nerf_sine_act_fwd(None, 16, 10, 16, P, 16, None) == -1
    assert lib.nerf_sine_act_fwd(P, 16, 10, 16, None, 16, None) == -1
    assert lib.nerf_sine_act_fwd(P, 8, 10, 16, P, 16, None) == -1           # ld_z < N
    assert lib.nerf_sine_act_fwd(P, 16, 10, 16, P, 8, None) == -1           # ld_y < N
    assert lib.nerf_sine_act_fwd(P, 16, -1, 16, P, 16, None) == -1
    assert lib.nerf_sine_act_fwd(None, 0, 0, 16, None, 0, None) == 0        # M == 0
    assert lib.nerf_sine_act_fwd(None, 0, 10, 0, None, 0, None) == 0        # N == 0
    # ---- nerf_sine_act_bwd(grad_y, ld_g, z, ld_z, M, N, grad_z, ld_dz, stream)
    assert lib.nerf_sine_act_bwd(None, 16, P, 16, 10, 16, P, 16, None) == -1
    assert lib.nerf_sine_act_bwd(P, 16, None, 16, 10, 16, P, 16, None) == -1
    assert lib.nerf_sine_act_bwd(P, 16, P, 16, 10, 16, None, 16, None) == -1
    assert lib.nerf_sine_act_bwd(P, 8, P, 16, 10, 16, P, 16, None) == -1    # ld_g < N
    assert lib.nerf_sine_act_bwd(P, 16, P, 8, 10, 16, P, 16, None) == -1    # ld_z < N
    assert lib.nerf_sine_act_bwd(P, 16, P, 16, 10, 16, P, 8, None) == -1    # ld_dz < N
    assert lib.nerf_sine_act_bwd(None, 0, None, 0, 0, 16, None, 0, None) == 0
    assert lib.nerf_sine_act_bwd(None, 0, None, 0, 10, 0, None, 0, None) == 0
    # ---- nerf_linear_sine_x3(segs, n_segs, M, W, ldw, N, bias, out, ldo, mode, y, ld_y, z, ld_z, stream)
    args = (None, 0, 10, P, 32, 8, None, P, 8)
    assert lib.nerf_linear_sine_x3(*args, 2, P, 8, None, 0, None) == -1                         # mode
    assert lib.nerf_linear_sine_x3(None, 0, 10, P, 32, 8, None, None, 8, 0, P, 8, None, 0, None) == -1   # out
    assert lib.nerf_linear_sine_x3(*args, 0, None, 8, None, 0, None) == -1                      # forward: y
    assert lib.nerf_linear_sine_x3(*args, 0, P, 4, None, 0, None) == -1                         # ld_y < N
    assert lib.nerf_linear_sine_x3(*args, 1, None, 0, None, 8, None) == -1                      # backward: z
    assert lib.nerf_linear_sine_x3(*args, 1, None, 0, P, 4, None) == -1                         # ld_z < N
    assert lib.nerf_linear_sine_x3(None, 0, 10, P, 32, 8, P, P, 8, 1, None, 0, P, 8, None) == -1   # backward with bias
    assert lib.nerf_linear_sine_x3(None, 0, 10, P, 32, 0, None, P, 8, 0, P, 8, None, 0, None) == -1   # N < 1
    assert lib.nerf_linear_sine_x3(None, 0, 0, P, 32, 8, None, P, 8, 0, P, 8, None, 0, None) == 0     # M == 0
    assert lib.nerf_linear_sine_x3(None, 0, 0, P, 32, 8, None, P, 8, 1, None, 0, P, 8, None) == 0
    n6 = (None, 0, 10, P, 32, 6, None, P, 8)
    assert lib.nerf_linear_sine_x3(*n6, 0, P, 8, None, 0, None) == -2                           # N % 4
    assert lib.nerf_linear_sine_x3(*n6, 1, None, 0, P, 8, None) == -2
    assert lib.nerf_linear_sine_x3(None, 0, 10, P, 32, 8, None, P + 4, 8, 0, P, 8, None, 0, None) == -2   # out alignment
    assert lib.nerf_linear_sine_x3(*args, 0, P, 10, None, 0, None) == -2                        # ld_y % 4
    assert lib.nerf_linear_sine_x3(*args, 0, P, 8, None, 0, None) == -1                         # no segments
