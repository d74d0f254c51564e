"""Times the person detector (include/poserisk_hip.h, section j8) on the GPU -> profiles/detector.json (or --out).

Per network input size (416 x 416, the reference's; 416 wide x 256 high, which suits 800 x 450 frames) and frame count (64, 256)
of 800 x 450 frames: each stage on its own (letterbox, network, post-processing: device events around `--repeats` calls after a
warm-up; SORT: host clock), frames/s of the whole chain (Detector.detect + sort.track_frames, host copies included), and the
network's achieved TFLOP/s -- the convolutions' multiply-adds computed from the layer shapes, over the network stage's time --
as a fraction of the 157.3 TFLOP/s fp32 MFMA peak.  That is a whole-stage rate over peak (it includes the concat kernels and
the gaps between 75 launches), not one kernel's share.
Yardsticks on the same box: tests/det_ref.py's float32 torch forward on 16 CPU threads, and, on the layer shapes
pr_conv2d_nhwc also accepts (Cout % 64 == 0; it runs them with plain ReLU, no residual), the encoder's tile kernel against the
detector's kernel through pr_det_conv_nhwc.

--precision bf16 times the bf16 detector alone; --precision both runs fp32 and bf16 back to back in ONE process on one box (the
yardstick for time is the fp32 path measured beside it, never a recorded number) and writes profiles/detector_bf16.json: the same
rows for both, the network's TFLOP/s against the 2.5 PFLOP/s bf16 MFMA peak and the 157.3 TFLOP/s fp32 one, the ratio per row, and
per distinct layer shape the bf16 kernel (pr_det_conv_nhwc_bf16) against the fp32 one (pr_det_conv_nhwc) on the same shape.

    python scripts/bench_detector.py [--frames 64 256] [--repeats 3] [--precision fp32|bf16|both] [--out ...] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
from poserisk_release_amd import detector, ops, sort, synth  # noqa: E402

PEAK_TFLOPS = 157.3
PEAK_BF16_TFLOPS = 2500.0


def network_flops(S_h, S_w):
    """Multiply-adds x 2 of the 75 convolutions for one frame."""
    return sum(2.0 * (S_h // l["down"]) * (S_w // l["down"]) * l["cout"] * l["cin"] * l["ksize"] ** 2
               for l in detector.yolo_layers() if l["type"] == detector.CONV)


def timed(fn, repeats, device):
    fn()
    torch.cuda.synchronize(device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize(device)
    return a.elapsed_time(b) / repeats


def bench_size(weights, size, n_frames, repeats, device, batch, precision="fp32"):
    det = detector.Detector(weights, img_size=size, device=device, max_batch=batch, precision=precision)
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (n_frames, 450, 800, 3), dtype=np.uint8)).to(device)
    chunks = [frames[i:i + batch] for i in range(0, n_frames, batch)]
    xs = [det.letterbox(c) for c in chunks]
    heads = [det.network(x) for x in xs]
    ms = {"letterbox": timed(lambda: [det.letterbox(c, out=x) for c, x in zip(chunks, xs)], repeats, device),
          "network": timed(lambda: [det.network(x, out=h) for x, h in zip(xs, heads)], repeats, device),
          "postprocess": timed(lambda: [det.postprocess(h, 0.1, 0.4) for h in heads], repeats, device)}
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    dets = det.detect(frames, conf_thres=0.1, nms_thres=0.4)
    t1 = time.perf_counter()
    tracks = sort.track_frames(dets)
    t2 = time.perf_counter()
    det.close()
    flops = network_flops(*size) * n_frames
    tflops = flops / (ms["network"] * 1e-3) / 1e12
    return {"precision": precision, "network_fraction_of_bf16_mfma_peak": tflops / PEAK_BF16_TFLOPS,
            "img_size": list(size), "frames": n_frames, "batch": batch, "stage_ms": ms, "sort_host_ms": (t2 - t1) * 1e3,
            "detect_with_host_copies_ms": (t1 - t0) * 1e3, "frames_per_s": n_frames / (t2 - t0),
            "frames_per_s_device_stages": n_frames / (sum(ms.values()) * 1e-3),
            "network_gflop_per_frame": network_flops(*size) / 1e9, "network_tflops": tflops, "network_fraction_of_fp32_mfma_peak": tflops / PEAK_TFLOPS,
            "detections": int(sum(len(d) for d in dets)), "tracks": len(tracks)}


def bench_cpu_reference(weights, size, n, threads=16):
    import det_ref
    x = np.random.default_rng(1).random((n, size[0], size[1], 4), dtype=np.float32)
    det_ref.forward(weights, x[:1], torch.float32, threads=threads)
    t0 = time.perf_counter()
    det_ref.forward(weights, x, torch.float32, threads=threads)
    dt = time.perf_counter() - t0
    return {"img_size": list(size), "frames": n, "threads": threads, "frames_per_s": n / dt, "tflops": network_flops(*size) * n / dt / 1e12}


def pack_one(w_oihw, bias):
    """One convolution in pr_det_fold_pack's layout: bias[cout_pad] then w[cout_pad][kpad]."""
    o, cin, k, _ = w_oihw.shape
    cout_pad, kpad = -(-o // 64) * 64, -(-(k * k * cin) // 32) * 32
    packed = np.zeros((cout_pad, 1 + kpad), np.float32)
    packed[:o, 0] = bias
    packed[:o, 1:1 + k * k * cin] = w_oihw.transpose(0, 2, 3, 1).reshape(o, -1)
    return np.concatenate([packed[:, 0], packed[:, 1:].ravel()])


def bench_layers(size, batch, repeats, device):
    """Every distinct convolution shape of the network that pr_conv2d_nhwc accepts: the encoder's kernel (ReLU) and the detector's
    (leaky) on the same input and weights."""
    seen, rows = set(), []
    rng = np.random.default_rng(2)
    for l in detector.yolo_layers():
        if l["type"] != detector.CONV or l["cout"] % 64 or l["cin"] % 4:
            continue
        gh, gw = size[0] // l["down"], size[1] // l["down"]
        key = (l["cin"], l["cout"], l["ksize"], l["stride"], gh, gw)
        if key in seen:
            continue
        seen.add(key)
        H, W = gh * l["stride"], gw * l["stride"]
        x = torch.from_numpy(rng.standard_normal((batch, H, W, l["cin"]), dtype=np.float32)).to(device)
        w = (rng.standard_normal((l["cout"], l["cin"], l["ksize"], l["ksize"]), dtype=np.float32) * np.float32(np.sqrt(2.0 / (l["cin"] * l["ksize"] ** 2))))
        b = rng.standard_normal(l["cout"], dtype=np.float32)
        _, ms_enc = ops.conv2d_nhwc(x, w, bias=b, stride=l["stride"], pad=l["ksize"] // 2, relu=True, repeats=repeats)
        packed = torch.from_numpy(pack_one(w, b)).to(device)
        y = torch.empty((batch, gh, gw, l["cout"]), device=device)
        ms_det = timed(lambda: ops.det_conv_nhwc(x, packed, l["cout"], l["ksize"], l["stride"], leaky=True, out=y), repeats, device)
        flops = 2.0 * batch * gh * gw * l["cout"] * l["cin"] * l["ksize"] ** 2
        rows.append({"cin": l["cin"], "cout": l["cout"], "k": l["ksize"], "stride": l["stride"], "grid": [gh, gw], "batch": batch,
                     "encoder_kernel_ms": ms_enc, "detector_kernel_ms": ms_det, "detector_over_encoder": ms_det / ms_enc,
                     "detector_tflops": flops / (ms_det * 1e-3) / 1e12, "encoder_tflops": flops / (ms_enc * 1e-3) / 1e12})
    return rows


def bench_layers_bf16(size, batch, repeats, device):
    """Every distinct convolution shape of the network the bf16 kernel runs (all but layer 0), head shapes included: the fp32
    kernel and the bf16 kernel on the same shape, each with the output type it has in the network."""
    import det_bf16_ref as br
    seen, rows = set(), []
    rng = np.random.default_rng(2)
    for i, l in enumerate(detector.yolo_layers()):
        if l["type"] != detector.CONV or i == 0:
            continue
        gh, gw = size[0] // l["down"], size[1] // l["down"]
        key = (l["cin"], l["cout"], l["ksize"], l["stride"], gh, gw)
        if key in seen:
            continue
        seen.add(key)
        H, W, k, o, cin = gh * l["stride"], gw * l["stride"], l["ksize"], l["cout"], l["cin"]
        x = rng.standard_normal((batch, H, W, cin), dtype=np.float32)
        w = rng.standard_normal((o, cin, k, k), dtype=np.float32) * np.float32(np.sqrt(2.0 / (cin * k * k)))
        b = rng.standard_normal(o, dtype=np.float32)
        p32 = pack_one(w, b)
        cout_pad = -(-o // 64) * 64
        blob = np.frombuffer(p32[:cout_pad].tobytes() + br.bf16_bits(p32[cout_pad:]).tobytes(), np.uint8).copy()
        x32, packed32, packed16 = torch.from_numpy(x).to(device), torch.from_numpy(p32).to(device), torch.from_numpy(blob).to(device)
        x16 = x32.to(torch.bfloat16)
        odt = torch.bfloat16 if l["bn"] else torch.float32
        y32 = torch.empty((batch, gh, gw, o), device=device)
        y16 = torch.empty((batch, gh, gw, o), device=device, dtype=odt)
        ms32 = timed(lambda: ops.det_conv_nhwc(x32, packed32, o, k, l["stride"], leaky=bool(l["bn"]), out=y32), repeats, device)
        ms16 = timed(lambda: ops.det_conv_nhwc_bf16(x16, packed16, o, k, l["stride"], bool(l["bn"]), None, odt, out=y16), repeats, device)
        flops = 2.0 * batch * gh * gw * o * cin * k * k
        rows.append({"cin": cin, "cout": o, "k": k, "stride": l["stride"], "grid": [gh, gw], "batch": batch, "fp32_kernel_ms": ms32,
                     "bf16_kernel_ms": ms16, "fp32_over_bf16": ms32 / ms16, "fp32_tflops": flops / (ms32 * 1e-3) / 1e12,
                     "bf16_tflops": flops / (ms16 * 1e-3) / 1e12})
    return rows


def main_precisions(a, device, weights, sizes):
    """--precision bf16 | both: the rows per precision, back to back in this process."""
    precisions = ("fp32", "bf16") if a.precision == "both" else (a.precision,)
    result = {"device": torch.cuda.get_device_name(0), "peak_fp32_mfma_tflops": PEAK_TFLOPS, "peak_bf16_mfma_tflops": PEAK_BF16_TFLOPS,
              "weights": "synth.yolo_weights(seed=11)", "frame_size": [450, 800], "runs": [], "network_fp32_over_bf16": [], "layers": []}
    for size in sizes:
        for n in ([8] if a.quick else a.frames):
            row = {}
            for precision in precisions:
                row[precision] = bench_size(weights, size, n, a.repeats, device, min(a.batch, n), precision)
                result["runs"].append(row[precision])
                print(json.dumps(row[precision]), flush=True)
            if len(row) == 2:
                result["network_fp32_over_bf16"].append({
                    "img_size": list(size), "frames": n, "network": row["fp32"]["stage_ms"]["network"] / row["bf16"]["stage_ms"]["network"],
                    "device_stages": row["bf16"]["frames_per_s_device_stages"] / row["fp32"]["frames_per_s_device_stages"]})
                print(json.dumps(result["network_fp32_over_bf16"][-1]), flush=True)
    result["layers"] = bench_layers_bf16(sizes[0], 2 if a.quick else 16, max(a.repeats, 5), device)
    out = a.out or os.path.join(REPO, "profiles", "detector_bf16.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"out": out, "layers": len(result["layers"])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="default: profiles/detector.json, or profiles/detector_bf16.json with --precision bf16 | both")
    ap.add_argument("--precision", choices=("fp32", "bf16", "both"), default="fp32")
    ap.add_argument("--quick", action="store_true", help="one small size, for a rehearsal")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector: no GPU visible (nothing is measured on the CPU)")
    device = torch.device("cuda", 0)
    weights = synth.yolo_weights(seed=11)
    sizes = [(64, 96)] if a.quick else [(416, 416), (256, 416)]
    if a.precision != "fp32":
        return main_precisions(a, device, weights, sizes)
    a.out = a.out or os.path.join(REPO, "profiles", "detector.json")
    result = {"device": torch.cuda.get_device_name(0), "peak_fp32_mfma_tflops": PEAK_TFLOPS, "weights": "synth.yolo_weights(seed=11)",
              "frame_size": [450, 800], "runs": [], "cpu_float32_reference": [], "layers": []}
    for size in sizes:
        for n in ([8] if a.quick else a.frames):
            result["runs"].append(bench_size(weights, size, n, a.repeats, device, min(a.batch, n)))
            print(json.dumps(result["runs"][-1]), flush=True)
        result["cpu_float32_reference"].append(bench_cpu_reference(weights, size, 2 if a.quick else 8))
        print(json.dumps(result["cpu_float32_reference"][-1]), flush=True)
    result["layers"] = bench_layers(sizes[0], 2 if a.quick else 16, max(a.repeats, 5), device)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"out": a.out, "layers": len(result["layers"])}))


if __name__ == "__main__":
    main()
