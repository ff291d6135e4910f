"""Packed-W2 storage (MIXDQ_FLAG_W2) against W4 and W8, on one MI355X, in one library:

  (a) per 2-bit shape family of weight_4.00 (N x K at 1024 px): us per launch for W8 / W4 / W2 storage of
      the same integers, batch 1 and 8, each on its automatic tile -- a captured graph of `iters` launches
      replayed `reps` times (median), so no host time is in the figure (tools/bench_gemm.py's method); the
      grouped k|v context projection (two members, the grouped launch's automatic tile) likewise;
      --sweep: W2 on every tile it takes, per family and batch (the data of select_cfg_w2);
  (b) the SDXL step (1024 px, batch 1, weight_4.00 + act_7.77, fused graph, hipGraph replay):
      w4_kernel=True against w4_kernel=True + w2_kernel=True, the two captured graphs replayed in
      alternation (median ms of the rounds, bench.py's timing of a replay);
  (c) static bytes of both converted networks, counted from their buffers.

Prints one JSON object (and writes it to --out)."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"

# (family, M per image, N, K): the 2-bit Linear families of weight_4.00 at 1024 px (M = rows per image)
FAMILIES = [("attn2.to_k|to_v 640", 76, 640, 2048), ("attn2.to_k|to_v 1280", 76, 1280, 2048),
            ("attn2.to_q 640", 4096, 640, 640), ("attn2.to_q 1280", 1024, 1280, 1280),
            ("attn2.to_out.0 640", 4096, 640, 640), ("attn2.to_out.0 1280", 1024, 1280, 1280),
            ("ff.net.0.proj 1280 (GEGLU)", 1024, 10240, 1280), ("ff.net.2 1280", 1024, 1280, 5120),
            ("ff.net.0.proj 640 (GEGLU)", 4096, 5120, 640), ("ff.net.2 640", 4096, 640, 2560)]


def _time(fn, iters=20, reps=7):
    """us per launch: `iters` launches captured in one graph, replayed `reps` times (median)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(out)


def _runs(fn):
    """The launch is accepted (a forced tile the format does not take raises before anything is queued)."""
    try:
        fn()
        torch.cuda.synchronize()
        return True
    except RuntimeError:
        return False


def kernels(batches, sweep):
    from mixdq_amd import _C as C
    from mixdq_amd.nn.utils import pack_w2, pack_w4
    rows = []
    tiles = [i for i in C.IGEMM_CONFIGS if i not in C.W2_INADMISSIBLE and i not in (70, 71)]
    g = torch.Generator().manual_seed(0)
    for fam, m1, N, K in FAMILIES:
        q = torch.randint(-2, 2, (N, K), generator=g, dtype=torch.int64).to(torch.int8)
        w = {8: q.to(DEV), 4: pack_w4(q).to(DEV), 2: pack_w2(q).to(DEV)}
        sc = torch.full((N,), 1e-4, device=DEV)
        b0 = q.float().sum(1).to(DEV)
        v, s = torch.ones(N, device=DEV), torch.ones(1, device=DEV)
        geglu = "GEGLU" in fam
        for B in batches:
            x = torch.randint(-128, 128, (B * m1, K), generator=g, dtype=torch.int64).to(torch.int8).to(DEV)
            row = dict(family=fam, batch=B, M=B * m1, N=N, K=K)
            si, zp = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)

            def launch(bits, cfg=0):
                kw = dict(_w4=bits == 4, _w2=bits == 2, _cfg=cfg)
                if geglu:
                    return lambda: C.qlinear_geglu(x, w[bits], sc, b0, None, si, zp, **kw)
                return lambda: C.qlinear_w8_a8_ohalf(x, w[bits], v, s, s, v, sc, b0, None, **kw)
            for bits in (8, 4, 2):
                row[f"w{bits}_us"] = round(_time(launch(bits)), 2)
                row[f"w{bits}_cfg"] = C.igemm_select_id(B * m1, N, K, K, w4=bits == 4, w2=bits == 2, geglu=geglu)
            if sweep:
                row["w2_sweep_us"] = {c: round(_time(launch(2, c)), 2) for c in tiles if _runs(launch(2, c))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    # the grouped k|v context projection (mixdq_qlinear_w8a8_grouped, the automatic tile: 37 for M <= 64, else 35)
    for N in (640, 1280):
        q = torch.randint(-2, 2, (N, 2048), generator=g, dtype=torch.int64).to(torch.int8)
        for B in batches:
            x = torch.randint(-128, 128, (B * 76, 2048), generator=g, dtype=torch.int64).to(torch.int8).to(DEV)
            row = dict(family=f"grouped attn2.to_k|to_v {N}", batch=B, M=B * 76, N=2 * N, K=2048)
            for bits, wt in ((8, q), (4, pack_w4(q)), (2, pack_w2(q))):
                members = [(wt.to(DEV).clone(), torch.zeros(N, device=DEV), torch.full((N,), 1e-4, device=DEV), None,
                            torch.empty(B * 76, N, dtype=torch.float16, device=DEV)) for _ in range(2)]
                t = C.GemmGroupTable(members, wbits=bits)
                row[f"w{bits}_us"] = round(_time(lambda: C.qlinear_grouped(x, t)), 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step(rounds, iters):
    from mixdq_amd import cfgs
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet

    class Args:
        w_config, a_config = cfgs.load("weight/weight_4.00"), cfgs.load("act/act_7.77")
    unet = build_unet(DEV)
    inputs = example_inputs(1, 128, DEV, seed=0)
    ckpt = calibrate(unet, [inputs])
    bos = precompute_bos(unet, inputs["encoder_hidden_states"])
    twin = copy.deepcopy(unet)
    quantize_unet(unet, Args, ckpt, bos=True, bos_dict=bos, w4_kernel=True)
    quantize_unet(twin, Args, ckpt, bos=True, bos_dict=bos, w4_kernel=True, w2_kernel=True)
    del ckpt
    nbytes = {}
    graphs = {}
    for name, u in (("w4", unet), ("w4+w2", twin)):
        u.set_fused(True)
        nbytes[name] = sum(b.numel() * b.element_size() for b in u.buffers())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(3):
                u(**inputs)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            out = u(**inputs)[0]
        graphs[name] = (g, out)
    for g, _ in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    same = bool(torch.equal(graphs["w4"][1], graphs["w4+w2"][1]))
    ms = {k: [] for k in graphs}
    for _ in range(rounds):                      # A/B alternation on the same box
        for k, (g, _) in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / iters)
    from mixdq_amd.nn import QuantizedLinear
    n_w2 = sum(bool(getattr(m, "w_packed2", False)) for m in twin.modules() if isinstance(m, QuantizedLinear))
    return dict(step_ms={k: round(statistics.median(v), 3) for k, v in ms.items()},
                step_ms_all={k: [round(x, 3) for x in v] for k, v in ms.items()},
                static_bytes=nbytes, saved_mb=round((nbytes["w4"] - nbytes["w4+w2"]) / 1e6, 1),
                w2_layers=n_w2, outputs_bit_equal=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="W2 on every tile it takes, per family and batch")
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), kernels=kernels((1, 8), a.sweep))
    if not a.no_step:
        res["step"] = step(a.rounds, a.iters)
        print(json.dumps(res["step"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
