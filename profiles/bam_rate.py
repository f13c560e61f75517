"""The reads stage from BAM against the reads stage from FASTQ, for the same reads: C3's read set (short reads, 150 bp, 10x of
5 Mbp) and C4's (long noisy reads, 5x), each written from one seed by this script's own writer as an inflated BAM stream and
as FASTQ text.  Writes profiles/bam_rate.json.

  BAM route    reset_reads + reads_bam_begin + add_reads_bam (pieces of --chunk bytes) + reads_bam_end   (bam.hip)
  FASTQ route  reset_reads + reads_text_begin + add_reads_text (the same pieces) + reads_text_end + the last record through
               the host reader                                                                             (reads_text.hip)
The FASTQ route is what a user does today after `samtools fastq`.  This commit does not touch it (reads_text.hip and the text
stream of phi_abi.hip are the parent's, byte for byte), so the yardstick is the parent's route measured in the same process.
Both start from INFLATED bytes in host memory (pageable; --pinned: pinned, written to the file --out names) -- the BGZF layer is the host pool's for both and is not timed -- and end when
the last hit flag is written (a device synchronise).  Timed by events on the context's stream and by the wall clock; the two
routes alternate, --repeats times each after one unrecorded round of both; the spread is that of the repeats.  Every round the
read counters and the hit vector of the two routes are compared.

Per kernel: `rocprofv3 --kernel-trace --stats -- python profiles/bam_rate.py --only bam --config C3` is a run of its own (nothing of it is
parsed here; profiles/bam_rate_kernels.txt is its summary, written by hand from the profiler's tables); the tiles confirmed / walked again come from phi_bam_info.

    python profiles/bam_rate.py [--repeats 5] [--config C3,C4] [--chunk 67108864] [--tile 0] [--only bam|fastq] [--pinned] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phi_amd                                                  # noqa: E402
from phi_amd import dist as pdist                              # noqa: E402
from phi_amd import ilp_index as H                             # noqa: E402
from phi_amd import synth                                      # noqa: E402

CODE = np.zeros(256, np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    CODE[_c] = _i
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b


def bam_stream(bases, off, rng):
    """An unaligned BAM (n_ref 0): per read the fixed part, a name r<i>, the packed sequence, qualities; a third of the reads
    stored reverse-complemented with 0x10."""
    out = [b"BAM\x01" + np.array([0, 0], "<i4").tobytes()]
    rev = rng.random(len(off) - 1) < 1 / 3
    lens = np.diff(off)
    if len(lens) and (lens == lens[0]).all() and lens[0] % 2 == 0 and len(lens) < 10 ** 7:
        # reads of one (even) length: every record at once, names r0000000 ...
        n, m = int(lens[0]), len(lens)
        s = bases[:m * n].reshape(m, n)
        s = np.where(rev[:, None], COMP[s[:, ::-1]], s)
        c = CODE[s]
        R = np.zeros((m, 36 + 9 + n // 2 + n), np.uint8)
        R[:, 0:4] = np.frombuffer(np.int32(32 + 9 + n // 2 + n).tobytes(), np.uint8)
        R[:, 4:12] = 255
        R[:, 12] = 9
        R[:, 14:16] = (72, 18)
        R[:, 18] = 4 | np.where(rev, 0x10, 0)
        R[:, 20:24] = np.frombuffer(np.int32(n).tobytes(), np.uint8)
        R[:, 24:32] = 255
        R[:, 36] = ord("r")
        idx = np.arange(m)
        for d in range(7):
            R[:, 43 - d] = 48 + (idx // 10 ** d) % 10
        R[:, 45:45 + n // 2] = c[:, 0::2] << 4 | c[:, 1::2]
        R[:, 45 + n // 2:] = 0x28
        return np.frombuffer(out[0] + R.tobytes(), np.uint8)
    for i in range(len(off) - 1):
        s = bases[off[i]:off[i + 1]]
        if rev[i]:
            s = COMP[s[::-1]]
        n = len(s)
        name = b"r%d\x00" % i
        c = CODE[s]
        if n & 1:
            c = np.append(c, 0)
        fixed = np.zeros(36, np.uint8)
        fixed[0:4] = np.frombuffer(np.int32(32 + len(name) + (n + 1) // 2 + n).tobytes(), np.uint8)
        fixed[4:8] = 255
        fixed[8:12] = 255
        fixed[12] = len(name)
        fixed[14:16] = (72, 18)
        fixed[18:20] = (4 | (0x10 if rev[i] else 0), 0)
        fixed[20:24] = np.frombuffer(np.int32(n).tobytes(), np.uint8)
        fixed[24:32] = 255
        out += [fixed.tobytes(), name, (c[0::2] << 4 | c[1::2]).astype(np.uint8).tobytes(), b"\x28" * n]
    return np.frombuffer(b"".join(out), np.uint8)


def fastq_text(bases, off):
    raw = bases.tobytes()
    return np.frombuffer(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, raw[off[i]:off[i + 1]], b"I" * int(off[i + 1] - off[i])) for i in range(len(off) - 1)), np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--config", default="C3,C4")
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--only", choices=["bam", "fastq"], default=None)
    ap.add_argument("--pinned", action="store_true", help="the host bytes of both routes in pinned memory (the command line pins its chunk buffers from the second chunk on)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bam_rate.json"))
    a = ap.parse_args()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    result = {"chunk_bytes": a.chunk, "tile_bytes": a.tile, "repeats": a.repeats, "host_memory": "pinned" if a.pinned else "pageable", "configs": {}}
    for name in a.config.split(","):
        gk, rk = synth.CONFIGS[name]
        g = synth.make_graph(**gk)
        bases, off, _ = synth.make_reads(g, **rk)
        bases = np.ascontiguousarray(np.frombuffer(bases, np.uint8) if not isinstance(bases, np.ndarray) else bases)
        off = np.ascontiguousarray(off, np.int64)
        bam = bam_stream(bases, off, np.random.default_rng(1))
        fq = fastq_text(bases, off)
        if a.pinned:
            bam, fq = (torch.from_numpy(x.copy()).pin_memory().numpy() for x in (bam, fq))
        n_reads, n_bases = len(off) - 1, int(off[-1])
        print(f"{name}: {n_reads} reads, {n_bases} bases; BAM {len(bam)} bytes, FASTQ {len(fq)} bytes", flush=True)
        ctx = phi_amd.Context(0)
        ctx.set_params(k=31, w=25, threshold=1.0, recombination=100)
        ctx.set_stream(stream.cuda_stream)
        A = g.arrays()
        ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
        torch.cuda.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record(stream)
            extra = fn()
            e1.record(stream)
            torch.cuda.synchronize()
            return dict(wall_ms=(time.perf_counter() - t0) * 1e3, event_ms=e0.elapsed_time(e1)), extra

        def run_bam():
            ctx.reset_reads()
            ctx.reads_bam_begin(a.chunk, a.tile)
            for i in range(0, len(bam), a.chunk):
                ctx.add_reads_bam(bam[i:i + a.chunk])
            return ctx.reads_bam_end()

        def run_fastq():
            ctx.reset_reads()
            ctx.reads_text_begin(a.chunk)
            for i in range(0, len(fq), a.chunk):
                assert not ctx.add_reads_text(fq[i:i + a.chunk])
            pending, taken = ctx.reads_text_end()
            ctx.add_reads(H.reads_of_text(pending, [], stream_offset=taken))
            return None

        def state():
            p, n = ctx.hits_buffer()
            return ctx.reads_stats(), torch.as_tensor(pdist.DevArray(p, n), device="cuda").cpu().numpy().copy()

        rows = {"bam": [], "fastq": []}
        info = None
        for rep in range(a.repeats + 1):
            st = {}
            if a.only != "fastq":
                t, info = timed(run_bam)
                st["bam"] = state()
                if rep:
                    rows["bam"].append(t)
            if a.only != "bam":
                t, _ = timed(run_fastq)
                st["fastq"] = state()
                if rep:
                    rows["fastq"].append(t)
            if len(st) == 2:
                assert st["bam"][0] == st["fastq"][0] and np.array_equal(st["bam"][1], st["fastq"][1]), (st["bam"][0], st["fastq"][0])
            print(rep, {k: v[-1] for k, v in rows.items() if v}, flush=True)
        cfg = {"n_reads": n_reads, "n_bases": n_bases, "bam_bytes": int(len(bam)), "fastq_bytes": int(len(fq)), "rows": rows, "bam_info": info}
        for k, v in rows.items():
            if v:
                ev = np.array([r["event_ms"] for r in v])
                cfg[k + "_event_ms"] = dict(median=float(np.median(ev)), min=float(ev.min()), max=float(ev.max()))
        if rows["bam"] and rows["fastq"]:
            cfg["bam_over_fastq"] = cfg["bam_event_ms"]["median"] / cfg["fastq_event_ms"]["median"]
        result["configs"][name] = cfg
        print(json.dumps({k: v for k, v in cfg.items() if k != "rows"}), flush=True)
        ctx.close()
    if a.only is None:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
