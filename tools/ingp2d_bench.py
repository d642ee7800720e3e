"""Timings of the 2-D hash-grid image fit (2d-ingp/main.py's configuration: 16 levels 16..2047,
T = 2^16, F = 2, Gigapixel(4, 256), batch 2560) on nerf_amd's kernels and on the eager torch
restatement (tests/_ingp2d_ref.py) on the same card, in alternating rounds: HIP events around
``--iters`` repetitions after warm-up, ``--rounds`` rounds each; median and range over the rounds.

  encoding   nerf_hashgrid2d_fwd and nerf_hashgrid2d_bwd (table gradient) at n = 2560 and n = 2^18
             (random pixel centres of the 2048 x 2048 image) against the restatement's forward and
             autograd backward
  render     Gigapixel.render(2048) against the restatement on the same chunks, with the achieved
             rate of the bytes the picture needs (per pixel: 8 B position, 4 corners x 16 levels x 8 B
             table rows, 12 B colour) against the HBM peak
  step       forward, MSE, backward and the Adam step at the training batch

Usage: python tools/ingp2d_bench.py [--rounds R] [--iters N] [--precision high|highest] [--only NAME]
Prints one line per measurement and a final JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-experiments_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s (MI355X, HBM3E)
L, T, F = 16, 2 ** 16, 2


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def alternate(name, ours, eager, rounds, iters, results, note=""):
    """ms per call of the two callables, alternating, after one warm-up call each."""
    ours(), eager()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(ours, iters))
        b.append(timed(eager, max(1, iters // 4)))
    ma, mb = statistics.median(a), statistics.median(b)
    results[name] = {"nerf_amd_ms": ma, "nerf_amd_range": [min(a), max(a)], "eager_ms": mb,
                     "eager_range": [min(b), max(b)], "ratio": mb / ma}
    print(f"{name:22s} nerf_amd {ma:9.4f} ms [{min(a):.4f} .. {max(a):.4f}]   eager {mb:9.4f} ms "
          f"[{min(b):.4f} .. {max(b):.4f}]   eager / nerf_amd {mb / ma:7.1f}x{note}", flush=True)
    return ma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default="high", choices=("highest", "high"))
    ap.add_argument("--only", default="", help="encoding | render | step")
    args = ap.parse_args()

    import nerf_amd  # noqa: F401
    import _ingp2d_ref as R
    from nerf_amd import kernels as K
    from nerf_amd import model_ingp2d as M

    torch.set_float32_matmul_precision(args.precision)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    enc = M.INGPEncoding(2048, 16, T, F, L)
    model = M.Gigapixel(4, 256, enc)
    with torch.no_grad():
        for e in enc.encodings:
            e.table.mul_(1e3)
    ref = R.RefGigapixel(4, 256, R.RefEncoding(enc.resolutions, T, F))
    ref.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    model, ref = model.to(dev), ref.to(dev)
    params = enc._hash_params()
    packed = enc.packed_table()
    ws = torch.empty((K.hashgrid2d_workspace_bytes(params) + 7) // 8, dtype=torch.int64, device=dev)
    grad = torch.empty_like(packed)
    centres = M.pixel_centres(2048, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    results = {"precision": args.precision, "rounds": args.rounds, "iters": args.iters}

    if args.only in ("", "encoding"):
        for n in (2560, 2 ** 18):
            x = centres[torch.randint(0, centres.shape[0], (n,), device=dev, generator=gen)].contiguous()
            out = torch.empty(n, L * F, device=dev)
            g = torch.randn(n, L * F, device=dev, generator=gen)
            fwd = lambda: K.hashgrid2d_fwd(params, packed, out, x, n)
            bwd = lambda: K.hashgrid2d_bwd(params, g, grad, ws, x, n)

            def both():
                fwd(), bwd()

            def eager_fwd():
                with torch.no_grad():
                    return ref.position_encoder(x)

            def eager_both():
                for p in ref.position_encoder.parameters():
                    p.grad = None
                ref.position_encoder(x).backward(g)

            alternate(f"enc fwd      n={n}", fwd, eager_fwd, args.rounds, args.iters, results)
            alternate(f"enc fwd+bwd  n={n}", both, eager_both, args.rounds, args.iters, results)
            results[f"enc bwd      n={n}"] = {"nerf_amd_ms": statistics.median(timed(bwd, args.iters)
                                                                                for _ in range(args.rounds))}
            print(f"enc bwd      n={n}      nerf_amd {results[f'enc bwd      n={n}']['nerf_amd_ms']:9.4f} ms", flush=True)

    if args.only in ("", "render"):
        chunk = 2 ** 20

        def eager_render():
            with torch.no_grad():
                return torch.cat([ref(centres[i:i + chunk]) for i in range(0, centres.shape[0], chunk)])

        it = max(2, args.iters // 5)
        ms = alternate("render 2048^2", lambda: model.render(2048, chunk), eager_render, args.rounds, it, results)
        need = centres.shape[0] * (8 + 4 * L * F * 4 + 12)
        rate = need / (ms * 1e-3)
        results["render 2048^2"].update(bytes=need, bytes_per_s=rate, hbm_share=rate / HBM_PEAK)
        print(f"render: {need / 1e9:.3f} GB needed, {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the "
              f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak (the MLP's activations stay out of this count)", flush=True)

    if args.only in ("", "step"):
        n = 2560
        x = centres[torch.randint(0, centres.shape[0], (n,), device=dev, generator=gen)].contiguous()
        y = torch.rand(n, 3, device=dev, generator=gen)
        opt = model.configure_optimizers()["optimizer"]
        opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            model.training_step((x, y)).backward()
            opt.step()

        def eager_step():
            opt_ref.zero_grad()
            torch.nn.functional.mse_loss(ref(x), y).backward()
            opt_ref.step()

        alternate(f"train step   n={n}", step, eager_step, args.rounds, args.iters, results)

    print(json.dumps(results))


if __name__ == "__main__":
    main()
