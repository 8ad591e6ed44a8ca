"""Ingest alone, host reader against device reader, on one BGZF FASTQ pair (the world of
scripts/e2e_bench.py scaled to `pairs` pairs, 2 M by default).

Host side: io.read_pairs (inflate + parse + pack on the host's cores, one figure: the reader does
not separate them) and pipeline.upload_reads (the copy to HBM).  Device side: io.read_pairs_device
with the reader's own seconds per phase (file read, host-to-device copy of the compressed bytes,
inflate + CRC32, parse, export) and pipeline.device_reads (the padding to the row stride the
device path uses).  Each side is run `--reps` times after one untimed warm-up run; the figures are
the medians.  The two results are compared byte for byte.  Prints one JSON line and writes it to
--out.

    python scripts/ingest_bench.py [--pairs 2000000] [--reps 3] [--out profiles/gpu_ingest/ingest_2m.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import afpkg  # noqa: E402,F401
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch-bytes", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpu_ingest", "ingest_2m.json"))
    args = ap.parse_args()
    import torch

    from anchored_fusion_amd import io as afio
    from anchored_fusion_amd import pipeline
    from e2e_bench import write_world
    folder = os.path.join(tempfile.gettempdir(), "af_ingest_bench")
    _, _, fq, L, t_gen = write_world(args.pairs, folder)
    dev = torch.device("cuda", 0)

    def host_once():
        t0 = time.perf_counter()
        names, reads, lens = afio.read_pairs(fq[1], fq[2])
        t1 = time.perf_counter()
        up = pipeline.upload_reads(reads, lens, 0)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        return dict(read_pairs=t1 - t0, upload=t2 - t1, total=t2 - t0), (names, reads, lens, up)

    def device_once():
        times = {}
        t0 = time.perf_counter()
        names, reads_t, lens_t = afio.read_pairs_device(fq[1], fq[2], 0, batch_bytes=args.batch_bytes, times=times)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        up = pipeline.device_reads(reads_t, lens_t)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        return dict(times, read_pairs_device=t1 - t0, pad=t2 - t1, total=t2 - t0), (names, reads_t, lens_t, up)

    _, host = host_once()
    _, devr = device_once()
    same = (host[0].arena == devr[0].arena and np.array_equal(host[0].off, devr[0].off)
            and np.array_equal(host[1], devr[1].cpu().numpy())
            and bool(torch.equal(host[3][0], devr[3][0])) and bool(torch.equal(host[3][1], devr[3][1])))
    n_pairs = host[1].shape[0] // 2
    del host, devr
    torch.cuda.empty_cache()
    runs = {"host": [], "device": []}
    for _ in range(args.reps):
        for side, fn in (("host", host_once), ("device", device_once)):
            t, keep = fn()
            runs[side].append(t)
            del keep
            torch.cuda.empty_cache()
    med = {side: {k: round(statistics.median(r[k] for r in rs), 4) for k in rs[0]} for side, rs in runs.items()}
    gz = os.path.getsize(fq[1]) + os.path.getsize(fq[2])
    res = {
        "leg": "ingest alone: one BGZF FASTQ pair -> rows, lens and names, the rows in HBM at the device path's stride",
        "pairs": n_pairs, "read_len": L, "fastq_gz_bytes": gz, "reps": args.reps, "equal": bool(same),
        "host_s": med["host"], "device_s": med["device"],
        "host_total_all": [round(r["total"], 4) for r in runs["host"]],
        "device_total_all": [round(r["total"], 4) for r in runs["device"]],
        "speedup_total": round(med["host"]["total"] / med["device"]["total"], 3),
        "device_inflate_gz_MBps": round(gz / 1e6 / max(med["device"]["inflate"], 1e-9), 1),
        "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or os.cpu_count(),
        "generate_s": round(t_gen, 1),
    }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    if not same:
        raise SystemExit("the device reader's result differs from the host reader's")


if __name__ == "__main__":
    main()
