"""4-bit activation quantizers (MIXDQ_FLAG_A4_*, a4_kernel=True) against 8-bit ones, on one MI355X, in one library:

  (a) each producer that honours the flag -- stand-alone quantize, LayerNorm + quantize, GEGLU + quantize, the
      attention kernels (77 and 1024 keys), to_q + cross-attention -- A8 against A4 on the same input at the
      batch-1 SDXL shapes: us per launch from a captured graph of `iters` launches replayed `reps` times (median;
      tools/bench_w2.py's method);
  (b) the SDXL step (1024 px, batch 1, weight_4.00 + act_7.77 and act_7.38, fused graph, hipGraph replay):
      w4_kernel + w2_kernel against w4_kernel + w2_kernel + a4_kernel, the two captured graphs replayed in
      alternation (median ms of the rounds);
  (c) static bytes of both converted networks, counted from their buffers;
  (d) kernels per step (one eager forward under torch.profiler: bench.py's count_kernels).

Prints one JSON object (and writes it to --out)."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_w2 import _time  # noqa: E402

DEV = "cuda:0"


def producers(iters):
    from mixdq_amd import _C as C
    g = torch.Generator().manual_seed(0)

    def f16(*shape):
        return (torch.randn(*shape, generator=g) * 1.2).half().to(DEV)

    si, zp = torch.full((), 6.0, device=DEV), torch.full((), -121.0, device=DEV)
    rows = []

    def row(name, fn8, fn4):
        r = dict(producer=name, a8_us=round(_time(fn8, iters), 2), a4_us=round(_time(fn4, iters), 2))
        rows.append(r)
        print(json.dumps(r), flush=True)

    x = f16(1, 4096, 640)
    row("quantize [4096, 640]", lambda: C.quantize_per_tensor_to_int8(x, si, zp),
        lambda: C.quantize_per_tensor_to_int8(x, si, zp, _abits=4))
    c = f16(1, 77, 2048)
    row("quantize BOS slice [76, 2048]", lambda: C.quantize_per_tensor_to_int8(c[:, 1:], si, zp),
        lambda: C.quantize_per_tensor_to_int8(c[:, 1:], si, zp, _abits=4))
    for M, D in ((4096, 640), (1024, 1280)):
        h = f16(M, D)
        gam, bet = f16(D), f16(D)
        qp = [(si, zp)] * 3
        row(f"layernorm_quantize [{M}, {D}] x3", lambda: C.layernorm_quantize(h, gam, bet, 1e-5, qp),
            lambda: C.layernorm_quantize(h, gam, bet, 1e-5, qp, _abits=(8, 4, 8)))
        hh = f16(M, 8 * D)
        row(f"geglu_quantize [{M}, {8 * D}]", lambda: C.geglu_quantize(hh, si, zp),
            lambda: C.geglu_quantize(hh, si, zp, _abits=4))
    for T, tkv, Cc in ((4096, 4096, 640), (1024, 77, 1280), (4096, 77, 640)):
        q, k, v = f16(1, T, Cc), f16(1, tkv, Cc), f16(1, tkv, Cc)
        row(f"attention_f16 T={T} Tkv={tkv} C={Cc}", lambda: C.attention_f16(q, k, v, Cc // 64, si, zp),
            lambda: C.attention_f16(q, k, v, Cc // 64, si, zp, _abits=4))
    for T, Cc in ((1024, 1280), (4096, 640)):
        a = torch.randint(-128, 128, (1, T, Cc), generator=g).to(torch.int8).to(DEV)
        w = torch.randint(-128, 128, (Cc, Cc), generator=g).to(torch.int8).to(DEV)
        sc, b0 = torch.full((Cc,), 1e-4, device=DEV), torch.zeros(Cc, device=DEV)
        k, v = f16(1, 77, Cc), f16(1, 77, Cc)
        row(f"qlinear_attention T={T} C={Cc}", lambda: C.qlinear_attention(a, w, sc, b0, k, v, si, zp),
            lambda: C.qlinear_attention(a, w, sc, b0, k, v, si, zp, _abits=4))
    return rows


def _kernels_per_step(u, inputs):
    import bench
    return bench.count_kernels(lambda: u(**inputs), torch.device(DEV))


def step(act, rounds, iters):
    from mixdq_amd import cfgs
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.nn import QuantizedConv2d, QuantizedLinear
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet

    class Args:
        w_config, a_config = cfgs.load("weight/weight_4.00"), cfgs.load(act)
    unet = build_unet(DEV)
    inputs = example_inputs(1, 128, DEV, seed=0)
    ckpt = calibrate(unet, [inputs])
    bos = precompute_bos(unet, inputs["encoder_hidden_states"])
    twin = copy.deepcopy(unet)
    quantize_unet(unet, Args, ckpt, bos=True, bos_dict=bos, w4_kernel=True, w2_kernel=True)
    quantize_unet(twin, Args, ckpt, bos=True, bos_dict=bos, w4_kernel=True, w2_kernel=True, a4_kernel=True)
    del ckpt
    nbytes, graphs, accel, n_kern = {}, {}, {}, {}
    for name, u in (("w4+w2", unet), ("w4+w2+a4", twin)):
        u.set_fused(True)
        nbytes[name] = sum(b.numel() * b.element_size() for b in u.buffers())
        accel[name] = sum(m.valid_for_acceleration for m in u.modules()
                          if isinstance(m, (QuantizedLinear, QuantizedConv2d)))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(3):
                u(**inputs)
        torch.cuda.current_stream().wait_stream(s)
        n_kern[name] = _kernels_per_step(u, inputs)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            out = u(**inputs)[0]
        graphs[name] = (g, out)
    for g, _ in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    o8, o4 = (graphs[k][1].float() for k in graphs)
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
    n_a4 = sum(m.valid_for_acceleration and m.act_bits == 4 for m in twin.modules() if isinstance(m, QuantizedLinear))
    return dict(act_config=act, step_ms={k: round(statistics.median(v), 3) for k, v in ms.items()},
                step_ms_all={k: [round(x, 3) for x in v] for k, v in ms.items()},
                static_bytes=nbytes, saved_mb=round((nbytes["w4+w2"] - nbytes["w4+w2+a4"]) / 1e6, 1),
                accelerated_layers=accel, a4_layers=n_a4, kernels_per_step=n_kern,
                output_mean_abs_diff=round(float((o8 - o4).abs().mean()), 5),
                output_mean_abs=round(float(o8.abs().mean()), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--acts", default="act/act_7.77,act/act_7.38")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), producers=producers(a.iters))
    if not a.no_step:
        res["steps"] = []
        for act in a.acts.split(","):
            r = step(act, a.rounds, a.iters)
            res["steps"].append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
