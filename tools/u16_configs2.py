#!/usr/bin/env python3
"""configs[2] (N = 100,000 x Mt = 500,000) whole on ONE GPU, X held as 16-bit
fixed point (100 GB; 400 GB as doubles, 200 GB as floats).  A measurement, not a
test: generate the methylation-like design on the device, simulate a phenotype,
run `--warmup` untimed and `--steps` timed VAMP iterations, print one JSON line
(iterations/s, device memory in use, the one-pass operator's time per launch and
its rate in stored bytes).

    python tools/u16_configs2.py [--N 100000] [--Mt 500000] [--steps 10] [--warmup 2] [--storage u16]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vampomi_amd as va  # noqa: E402


def mem_in_use():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        return None, None
    return total.value - free.value, total.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--Mt", type=int, default=500_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--storage", default="u16")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    out = {"N": a.N, "Mt": a.Mt, "storage": a.storage, "steps": a.steps, "warmup": a.warmup}
    t0 = time.perf_counter()
    with va.Data(a.N, a.Mt, storage=a.storage) as d:
        d.generate(a.seed, va.GEN_METH)
        d.sync()
        out["generate_s"] = round(time.perf_counter() - t0, 2)
        out["quant_stats"] = d.quant_stats()
        d.simulate_phen(a.seed)
        v = va.Vamp(d, va.VampOptions(max_iter=a.warmup + a.steps, stop_criteria_thr=0.0))
        v.begin()
        for _ in range(a.warmup):
            v.step()
        d.sync()
        d.set_timing(True, 4)
        d.reset_stats()
        t1 = time.perf_counter()
        for _ in range(a.steps):
            v.step()
        d.sync()
        dt = time.perf_counter() - t1
        s = d.stats()
        used, total = mem_in_use()
        v.end()
        out["iterations_per_s"] = round(a.steps / dt, 4)
        out["ms_per_step"] = round(1e3 * dt / a.steps, 2)
        out["device_bytes_in_use"], out["device_bytes_total"] = used, total
        out["x_bytes"] = 2 * d.M * d.ld if a.storage == "u16" else (4 if a.storage == "f32" else 8) * d.M * d.ld
        out["operator_kernel"] = d.kernel_name(3, 2)
        if s.op.timed:
            us = 1e3 * s.op.ms_timed / s.op.timed
            gbs = s.op.bytes_total / s.op.launches / (us * 1e-6) / 1e9
            out["operator"] = {"launches": s.op.launches, "us_per_launch": round(us, 1),
                               "stored_GB_per_s": round(gbs, 1), "frac_of_8TBs_peak": round(gbs / 8000.0, 4),
                               "elements_per_s": round(d.N * d.M / (us * 1e-6), 0)}
        out["a_passes_exec"] = s.a_passes_exec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
