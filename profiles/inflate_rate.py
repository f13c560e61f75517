#!/usr/bin/env python3
"""Rate of phi_inflate (gzip inflated on the GPU); prints one JSON line.

Input from a seed: --gb GB of synthetic FASTQ (150-base reads sampled from a random 4 Mbp backbone with 1 % substitutions,
Illumina-like qualities), compressed once as one gzip member at zlib level 6 and once at level 1 (by 16 host threads, pigz-style: 32-MB pieces
each with the 32 KB before it as dictionary, joined by sync flushes into one deflate stream).  For each level, the
median and spread of --reps calls after a warm-up:
  (a) device span: from the compressed bytes in device memory to the checked text in device memory (phi_inflate_info.device_ms,
      two HIP events; the span includes the host's work between kernels -- chain walk, allocations, copies of counts -- so
      it bounds the device time from above);
  (b) host bytes to host bytes: the whole call (upload, inflate, download) by the host clock;
  (c) the host inflater: zlib.decompress of the same file on one host core (the library the command line's host path uses);
  the chunks confirmed at their found start and the chunks decoded again.
The output is checked against zlib (CRC32) in the same run.  --sweep also times (a) at other chunk sizes (level 6).
--profile-run does one call per level and nothing else (for `rocprofv3 --kernel-trace --stats`).

    python profiles/inflate_rate.py [--gb 1.0] [--reps 5] [--sweep] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_fastq(n_bytes, seed=4903):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    qual = np.frombuffer(b"#+2:FFF", np.uint8)
    backbone = rng.choice(acgt, 4 << 20)
    L, rec = 150, 12 + 151 + 2 + 151
    n = n_bytes // rec + 1
    out = np.empty((n, rec), np.uint8)
    for b0 in range(0, n, 100_000):
        o = out[b0:b0 + 100_000]
        m = len(o)
        ids = np.arange(b0, b0 + m)
        o[:, 0], o[:, 1] = ord("@"), ord("r")
        for d in range(9):
            o[:, 10 - d] = ord("0") + (ids // 10 ** d) % 10
        o[:, 11] = 10
        pos = rng.integers(0, len(backbone) - L, m)
        seq = backbone[pos[:, None] + np.arange(L)[None, :]]
        sub = rng.random((m, L)) < 0.01
        seq[sub] = rng.choice(acgt, int(sub.sum()))
        o[:, 12:12 + L] = seq
        o[:, 12 + L] = 10
        o[:, 13 + L], o[:, 14 + L] = ord("+"), 10
        o[:, 15 + L:15 + 2 * L] = qual[np.minimum(rng.geometric(0.6, (m, L)), len(qual)) - 1]
        o[:, -1] = 10
    return out.reshape(-1)[:n_bytes].tobytes()


def gzip_one_member(text, level, piece=32 << 20, threads=16):
    """one gzip member compressed by `threads` host threads: each 32-MB piece is deflated with the 32 KB before it as its
    dictionary and ends on a sync flush (an empty stored block), so the pieces join into one deflate stream"""
    from concurrent.futures import ThreadPoolExecutor

    def one(i):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, *([text[max(0, i - 32768):i]] if i else []))
        last = i + piece >= len(text)
        return c.compress(text[i:i + piece]) + c.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)
    with ThreadPoolExecutor(threads) as ex:
        body = b"".join(ex.map(one, range(0, len(text), piece)))
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + (zlib.crc32(text)).to_bytes(4, "little") + (len(text) & 0xffffffff).to_bytes(4, "little")


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "all": [round(x, 4) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import phi_amd

    t0 = time.perf_counter()
    text = synth_fastq(int(a.gb * 1e9))
    crc = zlib.crc32(text)
    rec = {"text_bytes": len(text), "workload": "synthetic FASTQ, 150-base reads, one gzip member", "levels": {}}
    for level in (6, 1):
        comp = gzip_one_member(text, level)
        r = {"compressed_bytes": len(comp)}
        if a.profile_run:
            phi_amd.inflate(comp, as_array=True)
            continue
        out, info = phi_amd.inflate(comp, as_array=True)                            # warm-up, and the check
        assert len(out) == len(text) and zlib.crc32(out) == crc, "output differs from zlib"
        del out
        dev, e2e = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            out, info = phi_amd.inflate(comp, as_array=True)
            e2e.append(time.perf_counter() - t)
            dev.append(info["device_ms"] / 1e3)
            del out
        host = []
        for _ in range(a.reps if level == 6 else 1):
            t = time.perf_counter()
            h = zlib.decompress(comp, 31)
            host.append(time.perf_counter() - t)
            assert len(h) == len(text)
            del h
        gbps = lambda s: round(len(text) / s / 1e9, 3)                        # noqa: E731
        r.update({"chunk_bytes": phi_amd._capi.PHI_INFLATE_CHUNK_DEFAULT, "chunks": info["chunks"], "confirmed": info["confirmed"], "redecoded": info["redecoded"],
                  "marker_bytes": info["marker_bytes"],
                  "a_device_span_s": spread(dev), "a_GBps_median": gbps(statistics.median(dev)),
                  "b_host_to_host_s": spread(e2e), "b_GBps_median": gbps(statistics.median(e2e)),
                  "c_host_zlib_s": spread(host), "c_GBps_median": gbps(statistics.median(host)), "verified": "crc32 == zlib"})
        if a.sweep and level == 6:
            sw = {}
            for cb in (32 << 10, 48 << 10, 96 << 10, 128 << 10, 256 << 10):
                ms = []
                for _ in range(3):
                    out, info = phi_amd.inflate(comp, chunk_bytes=cb, as_array=True)
                    ms.append(info["device_ms"] / 1e3)
                    del out
                sw[str(cb)] = {"a_device_span_s_median": round(statistics.median(ms), 4), "a_GBps": gbps(statistics.median(ms)),
                               "confirmed": info["confirmed"], "redecoded": info["redecoded"], "chunks": info["chunks"]}
            r["chunk_sweep_level6"] = sw
        rec["levels"][str(level)] = r
        print(json.dumps({"level": level, **{k: v for k, v in r.items() if "GBps" in k}}), file=sys.stderr, flush=True)
    rec["wall_s"] = round(time.perf_counter() - t0, 1)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
