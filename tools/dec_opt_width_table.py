#!/usr/bin/env python3
"""The deferred output-layer launch alone, duration against width: aae_output_layer_step at a shape with
aae_set_split(w) for each width, timed by the library's own event pair around the launch (AAE_K_DEC_OPT), no step
running beside it (the critical launch of the same call is over before the deferred one starts, only the call's two
small reductions of a few us share the chip with its first tiles; the next call joins before it launches).  Prints us per launch, tiles per workgroup (the longest walk) and us per tile:
python tools/dec_opt_width_table.py [--items N] [--hidden 200,100] [--batch B] [--dtypes f32,bf16] [--steps K] [--widths ...]
A tile's cost that is flat in the width means the launch waits on latency per workgroup; one that grows with the width
means it is limited by what the whole chip shares (HBM)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "aae-recommender_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

WIDTHS = (32, 64, 96, 104, 112, 120, 128, 160, 192, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--hidden", default="200,100")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dtypes", default="f32")
    ap.add_argument("--widths", default=",".join(str(w) for w in WIDTHS))
    a = ap.parse_args()
    from aaerec._hip import HipAAE, DeviceCSR, K_DEC_OPT
    from tools.synth import throughput_corpus
    N, B = a.items, a.batch
    widths = [int(w) for w in a.widths.split(",")]
    ntiles = (N + 31) // 32
    X = throughput_corpus(8 * B, N, seed=1)
    rng = np.random.default_rng(0)
    print(f"{torch.cuda.get_device_name(0)}: N={N} ({ntiles} tiles of 32 items) B={B}, {a.steps} launches per width", flush=True)
    for dt in a.dtypes.split(","):
        for h in (int(x) for x in a.hidden.split(",")):
            m = HipAAE(N, h, 50, max_batch=B, rng_mode="device", dtype=dt)
            k = 1.0 / np.sqrt(h)
            m.load_params({"dec.lin3.weight": ((rng.random((N, h)) * 2 - 1) * k).astype(np.float32),
                           "dec.lin3.bias": np.zeros(N, dtype=np.float32)})
            csr = DeviceCSR(X, m.device)
            dh2 = torch.rand(B, h + 1, device=m.device)
            dh2[:, h] = 1.0
            m.dh2_rows(B)[:, :h + 1].copy_(dh2)
            n_cu = torch.cuda.get_device_properties(m.device).multi_processor_count
            print(f"{dt} hidden {h}:  width | us/launch | tiles/workgroup | us/tile | GB/s (24 B per parameter)", flush=True)
            for w in widths:
                m.set_split(w)
                for i in range(3):
                    m.output_layer_step(csr, (i % 8) * B, B)
                m.sync()
                torch.cuda.synchronize()
                m.profile_enable(True, kernels=(K_DEC_OPT,))
                for i in range(a.steps):
                    m.output_layer_step(csr, (i % 8) * B, B)
                m.sync()
                torch.cuda.synchronize()
                m.profile_enable(False)
                ms, n = m.profile_read(K_DEC_OPT)
                if not n:
                    raise SystemExit(f"no deferred launch was timed at width {w}: the output layer did not take its split form")
                us = ms / n * 1e3
                g = min(w, n_cu, ntiles)                     # (the library's own clamp: launch_output_deferred)
                tpw = (ntiles + g - 1) // g
                print(f"  {w:5d} | {us:9.1f} | {tpw:15d} | {us / tpw:7.2f} | {24.0 * N * (h + 1) / us / 1e3:6.0f}", flush=True)
            m.close()


if __name__ == "__main__":
    main()
