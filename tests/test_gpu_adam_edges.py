"""The fused Adam kernel (csrc/adam.hip, nerf_adam_step) and nerf_amd.FusedAdam at their edge shapes.

The C-ABI launches write into buffers guarded by a NaN pattern (tests/_guarded.py).  exp_avg and
exp_avg_sq use only adds and multiplies and must equal the fp32 restatement (tests/_adam_ref.py,
adam_ref32) bit for bit; the parameter is held elementwise to
  |p' - ref64| <= 4u |ref64| + 16u |step| (|m'| + |g'|) / denom + 1e-45,   u = 2^-24,
of which the fp32 restatement uses at most a quarter (tests/test_adam_prop_logic.py)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _adam_ref as A
from _guarded import GUARD, SENTINEL, Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import nerf_amd
    nerf_amd._lib.load()  # fail loudly if the HIP library is missing
    yield


def _guard(a):
    buf = Guarded(a.size)
    if a.size:
        buf.body.copy_(torch.from_numpy(a))
    return buf


def _alloc(case):
    """Per tensor guarded copies (p, g, m, v) of the case's arrays."""
    return [tuple(_guard(a) for a in t[:4]) for t in case.tensors]


def _batch(case, bufs, lo, hi):
    from nerf_amd import _lib
    b = _lib.NerfAdamBatch()
    b.n_tensors = hi - lo
    b.beta1, b.beta2, b.eps = case.beta1, case.beta2, case.eps
    b.one_minus_beta1, b.one_minus_beta2 = 1 - case.beta1, 1 - case.beta2
    for i in range(lo, hi):
        (p, g, m, v), t = bufs[i], case.tensors[i]
        n = t[0].size
        b.param[i - lo], b.grad[i - lo], b.exp_avg[i - lo], b.exp_avg_sq[i - lo] = \
            (p.ptr(), g.ptr(), m.ptr(), v.ptr()) if n else (None, None, None, None)
        b.numel[i - lo] = n
        b.step_size[i - lo], b.bc2_sqrt[i - lo], b.weight_decay[i - lo] = t[4], t[5], t[6]
    return b


def _read(case, bufs):
    """Check every guard, then per tensor the host copies (p', m', v')."""
    torch.cuda.synchronize()
    got = []
    for i, ((p, g, m, v), t) in enumerate(zip(bufs, case.tensors)):
        n_ = t[0].size
        for buf, what in ((p, "param"), (m, "exp_avg"), (v, "exp_avg_sq")):
            buf.check(f"{case.name}: tensor {i} {what}")
        # read only: its guards keep the pattern and its body the gradient's bits
        # (Guarded.check(written=False) is for a buffer that holds the pattern alone)
        gw = g.flat.cpu().numpy().view(np.uint32)
        assert np.all(gw[:GUARD] == SENTINEL) and np.all(gw[GUARD + n_:] == SENTINEL), f"tensor {i}: grad guards"
        assert np.array_equal(gw[GUARD:GUARD + n_], t[1].view(np.uint32)), f"tensor {i}: grad changed"
        got.append(tuple(b.body.cpu().numpy() for b in (p, m, v)))
    return got


def launch_c(case):
    """The whole case in one nerf_adam_step call on guarded buffers."""
    import nerf_amd
    lib = nerf_amd._lib.load()
    bufs = _alloc(case)
    b = _batch(case, bufs, 0, len(case.tensors))
    assert lib.nerf_adam_step(ctypes.byref(b), torch.cuda.current_stream().cuda_stream) == 0
    return _read(case, bufs)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def compare(case, got):
    """Every element of every tensor: m', v' bitwise against adam_ref32, p' within the bar of
    adam_ref64; where the restatement is NaN the kernel must be NaN (payloads are not compared)."""
    worst = 0.0
    for i, ((p, m, v), ((p64, m64, v64, bar), (p32, m32, v32))) in enumerate(zip(got, case.refs())):
        n = case.tensors[i][0].size
        assert p.shape == m.shape == v.shape == (n,)
        for name, a, r in (("exp_avg", m, m32), ("exp_avg_sq", v, v32)):
            nan = np.isnan(r)
            assert np.array_equal(np.isnan(a), nan), f"{case.name}: tensor {i} {name}: NaN at other elements"
            bad = np.flatnonzero((bits(a) != bits(r)) & ~nan)
            assert bad.size == 0, (f"{case.name}: tensor {i} (numel {n}) {name} differs from the fp32 restatement at "
                                   f"{bad.size} elements, first {bad[:4]}: {a[bad[:4]]} vs {r[bad[:4]]}")
        fin = np.isfinite(p64)
        assert np.array_equal(np.isfinite(p), fin), f"{case.name}: tensor {i} param: non-finite at other elements"
        assert np.array_equal(np.isnan(p), np.isnan(p64)), f"{case.name}: tensor {i} param: NaN at other elements"
        if fin.any():
            share = np.abs(p[fin].astype(np.float64) - p64[fin]) / bar[fin]
            worst = max(worst, float(share.max()))
            k = int(np.argmax(share))
            assert share[k] <= 1.0, (f"{case.name}: tensor {i} (numel {n}) param misses its bar {share[k]:.2f}-fold at "
                                     f"finite element {k}: {p[fin][k]!r} vs {p64[fin][k]!r}")
    print(f"{case.name}: param error at most {worst:.3f} of the bar")


def test_table_geometry_in_one_launch():
    """Numel 0, 1, 255 .. 257, 2047 .. 2049, 4096, 4097, 6145 and 3 with empty entries first, in the
    middle and last; every tensor has its own step_size, bc2_sqrt and weight_decay, so a block that
    picks a neighbour's entry, scalars or element range misses."""
    case = A.geometry_case()
    assert [t[0].size for t in case.tensors] == A.GEOMETRY_SIZES
    compare(case, launch_c(case))


def test_empty_tables_return_ok():
    import nerf_amd
    from nerf_amd import _lib
    lib = nerf_amd._lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    b = _lib.NerfAdamBatch()
    b.n_tensors = 0
    assert lib.nerf_adam_step(ctypes.byref(b), stream) == 0
    b.n_tensors = 5                                                # all empty: null pointers are fine
    assert lib.nerf_adam_step(ctypes.byref(b), stream) == 0
    b.n_tensors = _lib.NERF_ADAM_MAX_TENSORS
    assert lib.nerf_adam_step(ctypes.byref(b), stream) == 0
    torch.cuda.synchronize()


def test_full_table_of_48():
    """All 48 slots in one call, numel cycling 1, 2048, 2049, 300: slot 47 is updated like slot 0."""
    case = A.full_table_case()
    assert len(case.tensors) == 48
    got = launch_c(case)
    compare(case, got)
    assert not np.array_equal(bits(got[47][1]), bits(case.tensors[47][2])), "slot 47 was not updated"


@pytest.mark.parametrize("n_entries,launches", [(49, 2), (97, 3)])
def test_adam_step_chunks_update_every_entry_once(n_entries, launches, monkeypatch):
    """kernels.adam_step splits 49 / 97 entries into 2 / 3 launches; after one call every entry's m'
    equals one step of the restatement bitwise (a skipped entry keeps m, a doubly updated one has
    taken two steps)."""
    import nerf_amd
    from nerf_amd import kernels as K
    case = A.chunk_case(n_entries)
    bufs = _alloc(case)
    entries = [(p.body, g.body, m.body, v.body, t[4], t[5], t[6]) for (p, g, m, v), t in zip(bufs, case.tensors)]
    lib = nerf_amd._lib.load()
    calls = []

    class Counting:
        def __getattr__(self, name):
            return getattr(lib, name)

        def nerf_adam_step(self, batch, stream):
            calls.append(batch._obj.n_tensors)
            return lib.nerf_adam_step(batch, stream)

    monkeypatch.setattr(K._lib, "load", lambda: Counting())
    K.adam_step(entries, case.beta1, case.beta2, case.eps, torch.device(DEV))
    monkeypatch.undo()
    assert len(calls) == launches and sum(calls) == n_entries and max(calls) <= 48
    compare(case, _read(case, bufs))


@pytest.mark.parametrize("eps", [1e-5, 1e-8])
def test_value_edges(eps):
    """g = m = v = 0 leaves p as it was; v = 0 with m != 0 divides by eps alone; |g| from 1e-30 to
    1e18 (v' from underflow to 1e33)."""
    case = A.value_case(eps)
    got = launch_c(case)
    compare(case, got)
    p, m, v = got[0]
    p0, m0 = case.tensors[0][0], case.tensors[0][2]
    assert np.array_equal(bits(p[:1024]), bits(p0[:1024])) and not np.any(m[:1024]) and not np.any(v[:1024])
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    # v' = 0: the update is step * (m' / eps) exactly as the restatement has it, and it moved p
    assert not np.any(v[1024:2048]) and np.any(p[1024:2048] != p0[1024:2048])
    step = np.float32(case.tensors[0][4])
    m1 = m0[1024:2048] + np.float32(1 - case.beta1) * (np.float32(0) - m0[1024:2048])
    want = p0[1024:2048] + step * (m1 / (np.float32(0) / np.float32(case.tensors[0][5]) + np.float32(eps)))
    assert np.abs(p[1024:2048].astype(np.float64) - want).max() <= 4 * A.U * np.abs(want).max()


def test_nonfinite_gradients_stay_in_their_elements():
    """NaN and +-inf gradients at block and wave boundaries: p, m and v turn non-finite at exactly
    those elements; an infinite gradient leaves exp_avg = that infinity, exp_avg_sq = +inf and p NaN."""
    case = A.nonfinite_case()
    got = launch_c(case)
    compare(case, got)
    p, m, v = got[0]
    bad = np.zeros(A.VALUE_N, bool)
    bad[list(A.NONFINITE)] = True
    for a, what in ((p, "param"), (m, "exp_avg"), (v, "exp_avg_sq")):
        assert np.array_equal(~np.isfinite(a), bad), what
    for i, x in A.NONFINITE.items():
        if np.isinf(x):
            assert m[i] == x and v[i] == np.inf and np.isnan(p[i])
        else:
            assert np.isnan(m[i]) and np.isnan(v[i]) and np.isnan(p[i])


# ----------------------------------------------------------------------------- FusedAdam
def _shapes():
    """100 small parameters: a zero-element one, 2-D ones (one gets a non-contiguous gradient) and
    vectors of odd sizes."""
    shapes = [(0,), (5, 7), (3, 4)]
    shapes += [(1 + (7 * i) % 23,) if i % 4 else (2 + i % 5, 3 + i % 3) for i in range(97)]
    return shapes


GROUPS = ((0, 60, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-5)),
          (60, 85, dict(lr=5e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.02)),
          (85, 100, dict(lr=2e-3, betas=(0.95, 0.9999), eps=1e-6)))
NONCONTIG, SKIPPED, SKIP_STEP = 1, 61, 2


def _groups(params):
    return [dict(params=params[a:b], **kw) for a, b, kw in GROUPS]


def _params(seed=31):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in _shapes()]


def _grads(step):
    g = torch.Generator().manual_seed(1000 + step)
    out = []
    for i, s in enumerate(_shapes()):
        if i == SKIPPED and step == SKIP_STEP:
            out.append(None)
        elif i == NONCONTIG:
            out.append(torch.randn(s[::-1], generator=g).to(DEV).t())
        else:
            out.append(torch.randn(s, generator=g).to(DEV))
    return out


def _set_grads(params, step):
    for p, g in zip(params, _grads(step)):
        p.grad = None if g is None else g.clone(memory_format=torch.preserve_format)


def _assert_close_to_torch(pf, pt, of, ot):
    for i, (a, b) in enumerate(zip(pf, pt)):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=1e-6, atol=1e-7,
                                   err_msg=f"parameter {i}")
        sa, sb = of.state[a], ot.state[b]
        assert float(sa["step"]) == float(sb["step"])
        np.testing.assert_allclose(sa["exp_avg"].cpu().numpy(), sb["exp_avg"].cpu().numpy(), rtol=1e-6, atol=1e-7,
                                   err_msg=f"exp_avg {i}")
        np.testing.assert_allclose(sa["exp_avg_sq"].cpu().numpy(), sb["exp_avg_sq"].cpu().numpy(), rtol=1e-6,
                                   atol=1e-12, err_msg=f"exp_avg_sq {i}")


def test_fused_adam_three_batches_against_torch():
    """Three groups with their own betas and eps (three batches, the first of 60 tensors: two
    launches), weight decay in one, a zero-element parameter, a non-contiguous gradient, and a
    parameter without gradient on one step; 5 steps against torch.optim.Adam(foreach=False)."""
    from nerf_amd import FusedAdam
    base = _params()
    pf = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    pt = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    of, ot = FusedAdam(_groups(pf)), torch.optim.Adam(_groups(pt), foreach=False)
    for step in range(5):
        _set_grads(pf, step)
        _set_grads(pt, step)
        assert not pf[NONCONTIG].grad.is_contiguous()
        before = [p._version for p in pf]
        of.step()
        ot.step()
        for i, p in enumerate(pf):
            if p.grad is None:
                assert i == SKIPPED and step == SKIP_STEP and p._version == before[i]
            else:
                assert p._version > before[i], f"step {step}: parameter {i} kept its version"
    assert float(of.state[pf[SKIPPED]]["step"]) == 4 and float(of.state[pf[0]]["step"]) == 5
    _assert_close_to_torch(pf, pt, of, ot)


def _run_fused(steps, params=None, opt=None, first=0):
    from nerf_amd import FusedAdam
    if params is None:
        params = [torch.nn.Parameter(b.clone().to(DEV)) for b in _params()]
        opt = FusedAdam(_groups(params))
    for step in range(first, first + steps):
        _set_grads(params, step)
        opt.step()
    return params, opt


def test_state_dict_round_trip_is_bitwise():
    """3 steps, state_dict, a fresh FusedAdam with load_state_dict, 2 more steps: the parameters and
    the moments equal 5 uninterrupted steps bit for bit."""
    from nerf_amd import FusedAdam
    straight, os_ = _run_fused(5)
    part, op = _run_fused(3)
    sd = copy.deepcopy(op.state_dict())
    resumed = [torch.nn.Parameter(p.detach().clone()) for p in part]
    orr = FusedAdam(_groups(resumed))
    orr.load_state_dict(sd)
    _run_fused(2, resumed, orr, first=3)
    for i, (a, b) in enumerate(zip(straight, resumed)):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), i
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(os_.state[a][key].view(torch.int32), orr.state[b][key].view(torch.int32)), (i, key)
        assert float(os_.state[a]["step"]) == float(orr.state[b]["step"])


def test_torch_adam_state_continues_in_fused_adam():
    """A torch.optim.Adam state_dict after 3 steps, loaded into FusedAdam: 2 more steps of each agree."""
    from nerf_amd import FusedAdam
    base = _params()
    pt = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    ot = torch.optim.Adam(_groups(pt), foreach=False)
    for step in range(3):
        _set_grads(pt, step)
        ot.step()
    pf = [torch.nn.Parameter(p.detach().clone()) for p in pt]
    of = FusedAdam(_groups(pf))
    # a checkpoint's copy: load_state_dict keeps tensors that already have the parameter's dtype and
    # device, and the two optimizers must not share their moments
    of.load_state_dict(copy.deepcopy(ot.state_dict()))
    for step in range(3, 5):
        _set_grads(pt, step)
        ot.step()
    _run_fused(2, pf, of, first=3)
    _assert_close_to_torch(pf, pt, of, ot)


def test_unsupported_modes_raise():
    from nerf_amd import FusedAdam

    def one():
        p = torch.nn.Parameter(torch.randn(9, 4, device=DEV))
        p.grad = torch.randn(9, 4, device=DEV)
        return p

    for flag in ("amsgrad", "maximize", "capturable"):
        with pytest.raises(TypeError):
            FusedAdam([one()], **{flag: True})                     # the constructor does not take them
        p = one()
        opt = FusedAdam([p])
        opt.param_groups[0][flag] = True                           # as a loaded state_dict would set it
        keep = p.detach().clone()
        with pytest.raises(NotImplementedError):
            opt.step()
        assert torch.equal(p.detach(), keep)
    p = one()
    opt = FusedAdam([p])
    opt.load_state_dict(torch.optim.Adam([one()], amsgrad=True).state_dict())
    with pytest.raises(NotImplementedError):
        opt.step()
    p = one()
    p.grad = torch.randn(9, 4, device=DEV).to_sparse()
    keep = p.detach().clone()
    with pytest.raises(RuntimeError):
        FusedAdam([p]).step()
    assert torch.equal(p.detach(), keep)
