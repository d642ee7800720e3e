"""GaborF / SARF field networks without a GPU: construction and state-dict names against the
reference's fixtures (tests/golden/gaborf.npz, sarf.npz), plan lowering, the activations' algebra
(an fp64 restatement of csrc/param_act.h's formulas against the reference's fp64 results), and the
new C entry points' argument validation."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from _gabor_sarf_ref import INIT, KINDS, PARAMS, act_bwd, act_fwd, modules

FAMILIES = ["gaborf", "sarf"]
NEW_SYMBOLS = ["nerf_param_act_workspace", "nerf_param_act_fwd", "nerf_param_act_bwd", "nerf_linear_act_workspace",
               "nerf_linear_act_x3"]


@pytest.mark.parametrize("name", ["radiance", "proposal"])
@pytest.mark.parametrize("family", FAMILIES)
def test_construction_matches_reference_state(golden, family, name):
    """th.manual_seed(0) construction: the reference's key names (sarf's carry th.compile's
    ``_orig_mod.``) and initial values (sum and absolute sum of every tensor)."""
    mod, _ = modules(family)
    g = golden(family)
    torch.manual_seed(0)
    m = getattr(mod, "RadianceNetwork" if name == "radiance" else "ProposalNetwork")(*INIT[family])
    ref_keys = [str(k) for k in g[f"{name}.keys"]]
    if family == "sarf" and name == "radiance":      # sarf/model_radiance.py compiles its three Sequentials
        assert all("._orig_mod." in k for k in ref_keys)
    assert list(mod.strip_compile_prefix({k: None for k in ref_keys}).keys()) == list(m.state_dict().keys())
    for rk, (k, v) in zip(ref_keys, m.state_dict().items()):
        want = g[f"{name}.sdsum.{rk}"]
        got = np.array([v.double().sum().item(), v.double().abs().sum().item()])
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, err_msg=k)
    assert m.param_groups == []
    assert len(getattr(mod, "RadianceNetwork")(*INIT[family], 5e-4, 5e-5, 0, 0.5, 0.0).param_groups) == 2 \
        if name == "radiance" else True


@pytest.mark.parametrize("family", FAMILIES)
def test_activation_parameter_order(family):
    """parameters_gabor() / parameters_activation(): the reference's order (per activation module in
    construction order; Gabor: inv_standard_deviation, then spread)."""
    mod, act_cls = modules(family)
    m = mod.RadianceNetwork(*INIT[family])
    it = m.parameters_gabor() if family == "gaborf" else m.parameters_activation()
    acts = [x for x in m.modules() if isinstance(x, act_cls)]
    want = [getattr(a, p) for a in acts for p in PARAMS[family]]
    got = list(it)
    assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    lin = list(m.parameters_linear())
    assert [id(p) for p in lin] == [id(p) for x in m.modules() if isinstance(x, torch.nn.Linear)
                                    for p in (x.weight, x.bias)]
    assert {id(p) for p in m.parameters()} == {id(p) for p in lin + got}
    # the activation modules create their parameters in that order too (th.rand call order)
    a = act_cls(8, 0.5, 2.0)
    assert [n for n, _ in a.named_parameters()] == list(PARAMS[family])


@pytest.mark.parametrize("name", ["radiance", "proposal"])
@pytest.mark.parametrize("family", FAMILIES)
def test_plan_lowering(family, name):
    """Layer count, sources and residual as GARF's; params() = weight, bias, activation parameters."""
    from nerf_amd import mlp_fused, model_garf
    mod, act_cls = modules(family)
    m = getattr(mod, "RadianceNetwork" if name == "radiance" else "ProposalNetwork")(*INIT[family])
    garf = getattr(model_garf, "RadianceNetwork" if name == "radiance" else "ProposalNetwork")(0.5, 2.0)
    plan, gplan = m._get_plan(), garf._get_plan()
    linears = [x for x in m.modules() if isinstance(x, torch.nn.Linear)]
    assert [id(lp.module) for lp in plan.layers] == [id(x) for x in linears]
    assert plan.outputs == gplan.outputs and plan.column_outputs == gplan.column_outputs
    assert plan.contributors == gplan.contributors and plan.consumed == gplan.consumed
    want = []
    seqs = [m.model_density_1, m.model_density_2, m.model_color] if name == "radiance" else [m.model]
    for seq in seqs:
        mods = list(seq)
        for i, x in enumerate(mods):
            if isinstance(x, torch.nn.Linear):
                want += [x.weight, x.bias]
                if i + 1 < len(mods) and isinstance(mods[i + 1], act_cls):
                    want += [getattr(mods[i + 1], p) for p in PARAMS[family]]
    got = plan.params()
    assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    for lp, glp in zip(plan.layers, gplan.layers):
        assert lp.gauss is None and (lp.act is not None) == (glp.gauss is not None)
        assert (lp.residual, lp.residual_cols, lp.relu, lp.tanh) == (glp.residual, glp.residual_cols, False, False)
        assert [(s.kind, s.k_valid, s.k_pad, s.layer) for s in lp.sources] == \
            [(s.kind, s.k_valid, s.k_pad, s.layer) for s in glp.sources]
        if lp.act is not None:
            assert lp.act[0] == KINDS[family] and len(lp.act[1]) == len(PARAMS[family])
        lp.finalize("cpu")
        assert sorted(c for c in lp.col_map.tolist() if c >= 0) == list(range(lp.module.in_features))
    # the whole-network fused kernel has no such activation: it must refuse these plans
    assert all(mlp_fused._layer_shape(plan, i) is None for i, lp in enumerate(plan.layers) if lp.act is not None)
    assert not mlp_fused.eligible(plan, 1 << 16)


@pytest.mark.parametrize("family", FAMILIES)
def test_restated_formulas_reproduce_reference_fp64(golden, family):
    """csrc/param_act.h's algebra, restated in fp64 torch, against the reference module run in fp64."""
    g = golden(family)
    z = torch.from_numpy(g["act.z"]).double()
    gy = torch.from_numpy(g["act.gy"]).double()
    ps = [torch.from_numpy(g[f"act.{p}"]).double() for p in PARAMS[family]]
    got = (act_fwd(family, z, *ps),) + tuple(act_bwd(family, gy, z, *ps))
    names = ["y", "dz"] + [f"d_{p}" for p in PARAMS[family]]
    for n, t in zip(names, got):
        want = g[f"act.{n}.f64"]
        assert want.dtype == np.float64
        scale = np.abs(want).max()
        assert np.abs(t.numpy() - want).max() <= 1e-12 * scale, n
    if family == "sarf":
        assert (got[1][0, :2] == 0).all()          # dz at z = +-0


def test_new_symbols_declared_and_exported():
    from nerf_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_amd.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define\s+NERF_ACT_GABOR\s+1\b", src) and re.search(r"#define\s+NERF_ACT_SARF\s+2\b", src)
    assert (_lib.NERF_ACT_GABOR, _lib.NERF_ACT_SARF) == (1, 2)
    # the package exports the two activation modules
    import nerf_amd
    from nerf_amd import GaborAct, SarfAct
    assert GaborAct is modules("gaborf")[1] and SarfAct is modules("sarf")[1]
    assert nerf_amd.GaussAct is not None and not hasattr(nerf_amd, "NoSuchAct")
    assert lib.nerf_abi_version() == 10


def test_argument_validation_returns_status_without_launch():
    from nerf_amd import _lib
    lib = _lib.load()
    P = 256        # any non-null, 16-byte aligned address: nothing is dereferenced before the checks
    # ---- nerf_param_act_fwd(kind, z, ld_z, p0, p1, M, N, y, ld_y, stream)
    for kind in (0, 3, -1):
        assert lib.nerf_param_act_fwd(kind, P, 16, P, P, 10, 16, P, 16, None) == -1
        assert lib.nerf_param_act_workspace(kind, 1000, 64) == 0
    assert lib.nerf_param_act_fwd(1, None, 16, P, P, 10, 16, P, 16, None) == -1
    assert lib.nerf_param_act_fwd(1, P, 16, P, None, 10, 16, P, 16, None) == -1       # Gabor needs spread
    assert lib.nerf_param_act_fwd(2, P, 16, None, None, 10, 16, P, 16, None) == -1
    assert lib.nerf_param_act_fwd(2, P, 8, P, None, 10, 16, P, 16, None) == -1         # ld_z < N
    assert lib.nerf_param_act_fwd(1, P, 16, P, P, 10, 16, P, 8, None) == -1            # ld_y < N
    assert lib.nerf_param_act_fwd(1, None, 16, None, None, 0, 16, None, 16, None) == 0  # M == 0
    assert lib.nerf_param_act_fwd(2, None, 0, None, None, 10, 0, None, 0, None) == 0    # N == 0
    # ---- nerf_param_act_bwd(kind, gy, ld_g, z, ld_z, p0, p1, M, N, dz, ld_dz, g0, g1, acc, ws, bytes, stream)
    assert lib.nerf_param_act_workspace(1, 1000, 64) >= 2 * 2 * 64 * 8
    assert lib.nerf_param_act_workspace(2, 1000, 64) >= 2 * 64 * 8
    assert lib.nerf_param_act_workspace(1, 1000, 64) > lib.nerf_param_act_workspace(2, 1000, 64)
    assert lib.nerf_param_act_bwd(0, P, 16, P, 16, P, P, 10, 16, P, 16, P, P, 0, P, 1 << 20, None) == -1
    assert lib.nerf_param_act_bwd(1, P, 16, P, 16, P, P, 10, 16, P, 16, P, None, 0, P, 1 << 20, None) == -1
    assert lib.nerf_param_act_bwd(2, P, 16, P, 16, P, None, 10, 16, P, 16, None, None, 0, P, 1 << 20, None) == -1
    assert lib.nerf_param_act_bwd(2, None, 16, P, 16, P, None, 10, 16, P, 16, P, None, 0, P, 1 << 20, None) == -1
    assert lib.nerf_param_act_bwd(2, P, 16, P, 16, P, None, 10, 16, P, 8, P, None, 0, P, 1 << 20, None) == -1
    assert lib.nerf_param_act_bwd(1, P, 16, P, 16, P, P, 10, 16, P, 16, P, P, 0, None, 0, None) == -4
    short = lib.nerf_param_act_workspace(1, 10, 16) - 1
    assert lib.nerf_param_act_bwd(1, P, 16, P, 16, P, P, 10, 16, P, 16, P, P, 0, P, short, None) == -4
    assert lib.nerf_param_act_bwd(2, None, 0, None, 0, None, None, 10, 0, None, 0, None, None, 0, None, 0, None) == 0
    # ---- nerf_linear_act_x3(kind, segs, n_segs, M, W, ldw, N, bias, out, ldo, mode, p0, p1, y, ld_y, z, ld_z,
    #                         g0, g1, acc, ws, bytes, stream)
    assert lib.nerf_linear_act_workspace(0, 1000, 64) == 0
    assert lib.nerf_linear_act_workspace(1, 1000, 64) >= 2 * 4 * 64 * 8
    args = (None, 0, 10, P, 32, 8, None, P, 8)
    assert lib.nerf_linear_act_x3(0, *args, 0, P, P, P, 8, None, 0, None, None, 0, None, 0, None) == -1   # kind
    assert lib.nerf_linear_act_x3(1, *args, 2, P, P, P, 8, None, 0, None, None, 0, None, 0, None) == -1   # mode
    assert lib.nerf_linear_act_x3(1, *args, 0, P, None, P, 8, None, 0, None, None, 0, None, 0, None) == -1  # spread
    assert lib.nerf_linear_act_x3(2, *args, 0, P, None, None, 8, None, 0, None, None, 0, None, 0, None) == -1  # y
    assert lib.nerf_linear_act_x3(2, *args, 0, P, None, P, 4, None, 0, None, None, 0, None, 0, None) == -1  # ld_y < N
    assert lib.nerf_linear_act_x3(1, *args, 1, P, P, None, 0, P, 8, P, None, 0, None, 0, None) == -1      # grad_p1
    empty = (None, 0, 0, P, 32, 8, None, P, 8)
    assert lib.nerf_linear_act_x3(2, *empty, 0, P, None, P, 8, None, 0, None, None, 0, None, 0, None) == 0
    n6 = (None, 0, 10, P, 32, 6, None, P, 8)
    assert lib.nerf_linear_act_x3(2, *n6, 0, P, None, P, 8, None, 0, None, None, 0, None, 0, None) == -2   # N % 4
    assert lib.nerf_linear_act_x3(2, *args, 1, P, None, None, 0, P, 8, P, None, 0, None, 0, None) == -4   # workspace
    assert lib.nerf_linear_act_x3(1, *args, 1, P, P, None, 0, P, 8, P, P, 0, P, 8, None) == -4            # short
