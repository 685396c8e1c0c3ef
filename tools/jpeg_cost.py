"""What decoding JPEG files costs: Pillow on the host against spe_amd.jpeg (host entropy pass + two launches), for a batch of two
375 x 500 4:2:0 files (the recorded one of tests/golden/jpeg_voc.pt, twice) -> profiles/jpeg_decode.txt.

    python tools/jpeg_cost.py --out profiles/jpeg_decode.txt
    rocprofv3 --kernel-trace --stats -d build/jpeg_trace --output-format csv -- python tools/jpeg_cost.py --trace-run
    python tools/jpeg_cost.py --kernel-stats build/jpeg_trace --out build/jpeg_kernels.txt      # needs no GPU

(a) Pillow's decode + np.asarray + the upload of the RGB is the yardstick; (b) entropy_decode alone, 1 and 4 threads; (c) upload +
the two launches; (d) each kernel's bytes against the HBM bound, with the kernel times of the trace run.  Host numbers are wall
clock around work that ends in a device synchronise where a device is involved."""
import argparse
import csv
import glob
import io
import os
import statistics
import sys
import time
import warnings
from concurrent.futures import ThreadPoolExecutor

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 6.3e12          # bytes / s: the measured copy rate the other profiles use as the bound
B = 2


def spread(ts):
    ts = sorted(ts)
    return f"{statistics.median(ts) * 1e3:.3f} ms (p10 .. p90: {ts[len(ts) // 10] * 1e3:.3f} .. {ts[(9 * len(ts)) // 10] * 1e3:.3f}, n = {len(ts)})"


def timed(fn, n, warm):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return out


def traffic(infos):
    """Bytes each kernel has to move for these images: (pass A, pass B)."""
    a = b = 0
    for i in infos:
        a += i.nblocks * 64 * 2 + 384 + i.nblocks * 64                  # coefficients and tables in, planes out
        b += i.nblocks * 64 + i.width * i.height * 3                      # planes in, RGB out
    return a, b


def kernel_section(stats_dir, infos):
    files = glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return [f"(d) no kernel statistics under {stats_dir}"]
    rows = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            rows[r["Name"]] = r
    a, b = traffic(infos)
    out = ["(d) kernel durations from a rocprofv3 --kernel-trace --stats run of its own, against the bytes each kernel must move "
           f"(HBM bound at {HBM / 1e12:.1f} TB/s):"]
    for key, nbytes in (("jd_idct_kernel", a), ("jd_colour_kernel", b)):
        hit = [r for n, r in rows.items() if key in n]
        if not hit:
            out.append(f"    {key}: not in the trace")
            continue
        r = hit[0]
        avg, bound = float(r["AverageNs"]) / 1e3, nbytes / HBM * 1e6
        out.append(f"    {key:18s} {avg:6.1f} us average ({float(r['MinNs']) / 1e3:.1f} .. {float(r['MaxNs']) / 1e3:.1f}, {r['Calls']} calls); "
                   f"must move {nbytes / 1e6:.2f} MB = {bound:.2f} us at the bound = {100 * bound / avg:.0f} % of its time")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--trace-run", action="store_true", help="only 50 reconstruct calls, for a kernel trace")
    ap.add_argument("--kernel-stats", help="directory of a rocprofv3 --kernel-trace --stats run: print section (d) from it")
    args = ap.parse_args()
    import jpeg_cases as C
    from spe_amd import jpeg as J
    warnings.filterwarnings("ignore", message="The given NumPy array is not writable")      # np.asarray of a PIL image: only read here
    data = C.load("jpeg_voc")["data"].numpy().tobytes()
    datas = [data] * B
    infos = [J.probe(d) for d in datas]
    lines = []
    if args.kernel_stats:
        lines = kernel_section(args.kernel_stats, infos)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("jpeg_cost: no GPU - the measurement does not fall back")
        dev = torch.device("cuda:0")
        sync = torch.cuda.synchronize
        bufs = [torch.empty((J.record_elems(i),), dtype=torch.int16, pin_memory=True) for i in infos]
        coeffs = [J.entropy_decode(d, out=b) for d, b in zip(datas, bufs)]
        if args.trace_run:
            for _ in range(50):
                J.reconstruct(coeffs, dev)
            sync()
            return
        lines.append(f"# Decoding a batch of {B} files of {infos[0].width} x {infos[0].height}, 4:2:0, quality 90, {len(data)} bytes each "
                     f"({infos[0].nblocks} blocks): Pillow on the host against spe_amd.jpeg")
        lines.append(f"# (tools/jpeg_cost.py; wall clock around synchronised work, 20 warm-up + {args.steps} timed batches; torch {torch.__version__}, "
                     f"{os.cpu_count()} CPUs visible, {torch.cuda.get_device_name(0)})")
        try:
            import numpy as np
            import PIL
            from PIL import Image

            def pil_decode():
                return [np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in datas]

            def pil_all():
                ts = [torch.from_numpy(a).to(dev, non_blocking=True) for a in pil_decode()]
                sync()
                return ts
            lines.append(f"(a) Pillow {PIL.__version__}, the yardstick: decode + np.asarray alone {spread(timed(pil_decode, args.steps, 20))}")
            lines.append(f"    with the upload of the RGB and the synchronise: {spread(timed(pil_all, args.steps, 20))}")
            ref = pil_all()
            same = all(torch.equal(a, b) for a, b in zip(ref, J.decode_batch(datas, dev)))
            lines.append(f"    output equal to decode_batch's: {'yes' if same else 'NO'}")
        except ImportError:
            lines.append("(a) Pillow does not import on this machine: not measured here")
        one = timed(lambda: [J.entropy_decode(d, out=b) for d, b in zip(datas, bufs)], args.steps, 20)
        lines.append(f"(b) entropy_decode alone (probe + Huffman pass into reused pinned buffers), 1 thread: {spread(one)}")
        with ThreadPoolExecutor(max_workers=4) as ex:
            four = timed(lambda: list(ex.map(lambda p: J.entropy_decode(p[0], out=p[1]), zip(datas, bufs))), args.steps, 20)
        lines.append(f"    on a pool of 4 threads (a batch of {B} keeps {B} of them busy): {spread(four)}")

        def device_part():
            r = J.reconstruct(coeffs, dev)
            sync()
            return r
        lines.append(f"(c) upload of {sum(c.record.numel() * 2 for c in coeffs) / 1e6:.2f} MB of coefficients + the two launches + synchronise: "
                     f"{spread(timed(device_part, args.steps, 20))}")
        ev = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            J.reconstruct(coeffs, dev)
            b.record()
            ev.append((a, b))
        sync()
        lines.append(f"    the same by device events (upload, descriptor copy and both kernels): {spread([a.elapsed_time(b) / 1e3 for a, b in ev])}")
        whole = timed(lambda: (J.decode_batch(datas, dev, threads=4), sync()), args.steps, 20)
        lines.append(f"    decode_batch, everything (threads = 4): {spread(whole)}")
        ta, tb = traffic(infos)
        lines.append(f"(d) bytes the kernels must move per batch: pass A {ta / 1e6:.2f} MB = {ta / HBM * 1e6:.2f} us at the HBM bound of {HBM / 1e12:.1f} TB/s, "
                     f"pass B {tb / 1e6:.2f} MB = {tb / HBM * 1e6:.2f} us; kernel times: the trace run below")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
