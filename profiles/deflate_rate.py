"""BGZF written on the device (phi_deflate_bgzf, deflate.hip): ratio, rate and what `--bgzf` costs a command.
Run by hand on the MI355X; writes profiles/deflate_rate.json, everything taken in one run:

  (i)   per text -- the MHC-CHM13 FASTA of tests/golden/data (4.9 MB), a synthetic FASTA of 176 MB (the segments of a graph of
        the native generator, 173.8 M bases in 80-column lines: random bases, what a haplotype of that size compresses like) and
        the VCF of C2's `--calls` -- the device_ms of phi_deflate_info, the wall time of phi_amd.deflate_bgzf through Python
        (upload, download and the copy into bytes included), GB/s of input by both, and the ratio beside zlib's levels 1 and 6
        on the same 65 280-byte blocks
  (ii)  zlib's time for the same work on one core (level 1; level 6 on the texts below 20 MB)
  (iii) the stages "FASTA write" and "calls (device) + VCF write" of one `PHI --calls` command at C2, without and with --bgzf

    python profiles/deflate_rate.py [--repeats 3] [--no-large] [--no-cli] [--out FILE]
"""
import argparse
import ctypes as C
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np
import torch  # noqa: F401  (its HIP runtime initialises first, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import phi_amd                                                  # noqa: E402
from phi_amd import ilp_index as H                              # noqa: E402
from phi_amd import synth                                       # noqa: E402

PHI = os.path.join(ROOT, "phi_amd", "PHI")
DATA = os.path.join(ROOT, "tests", "golden", "data")
STAGE = re.compile(r"\[phi timing\] main: stage (.+?)\s+[\d.]+ ->\s+[\d.]+ s\s+\(\s*([\d.]+) ms\)")
BLOCK = 65280


def fasta_text(name, seq):
    L = H.host_lib()
    seq = np.ascontiguousarray(seq, np.uint8)
    text, n = C.c_void_p(), C.c_int64()
    assert L.phi_format_fasta(name, seq.ctypes.data_as(C.c_char_p), len(seq), C.byref(text), C.byref(n)) == 0
    try:
        return C.string_at(text, n.value)
    finally:
        L.phi_host_free_text(text)


def zlib_blocks(text, level):
    """(bytes, seconds) of zlib on one core over the same blocks, framing counted as BGZF's"""
    t0, total = time.perf_counter(), 28
    for i in range(0, len(text), BLOCK):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(text[i:i + BLOCK])) + len(c.flush()) + 26
    return total, time.perf_counter() - t0


def measure(name, text, repeats):
    row = {"text": name, "bytes": len(text), "blocks": -(-len(text) // BLOCK), "runs": []}
    out = None
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        out, info = phi_amd.deflate_bgzf(text, with_info=True)
        t1 = time.perf_counter()
        if rep:                                                 # (the first call is the warm-up)
            row["runs"].append({"device_ms": info["device_ms"], "wall_ms": (t1 - t0) * 1e3})
    assert gzip.decompress(out) == text
    row.update({k: int(info[k]) for k in ("out_bytes", "stored_blocks", "matches", "match_bytes")})
    dev, wall = (float(np.median([r[k] for r in row["runs"]])) for k in ("device_ms", "wall_ms"))
    row["median"] = {"device_ms": dev, "wall_ms": wall, "device_gb_per_s": len(text) / dev / 1e6, "wall_gb_per_s": len(text) / wall / 1e6}
    row["ratio"] = len(out) / len(text)
    z1, s1 = zlib_blocks(text, 1)
    row["zlib_level_1"] = {"ratio": z1 / len(text), "one_core_ms": s1 * 1e3}
    if len(text) < 20_000_000:
        z6, s6 = zlib_blocks(text, 6)
        row["zlib_level_6"] = {"ratio": z6 / len(text), "one_core_ms": s6 * 1e3}
    return row


def cli_stages(args):
    r = subprocess.run([PHI] + args, capture_output=True, text=True, timeout=900, env=dict(os.environ, PHI_TIMING="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    ms = {m.group(1).strip(): float(m.group(2)) for m in STAGE.finditer(r.stderr)}
    return {"fasta_write_ms": ms["FASTA write"], "calls_and_vcf_write_ms": ms["calls (device) + VCF write"],
            "bgzf_lines": [re.sub(r"written to \S*/", "written to ", ln.split("] ", 1)[-1]) for ln in r.stderr.splitlines() if "BGZF: " in ln]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deflate_rate.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "texts": []}

    def add(name, text):
        out["texts"].append(measure(name, text, a.repeats))
        print(json.dumps({k: v for k, v in out["texts"][-1].items() if k != "runs"}), flush=True)

    with gzip.open(os.path.join(DATA, "MHC-CHM13.0.fa.gz"), "rb") as f:
        lines = f.read().split(b"\n")
    add("MHC-CHM13 FASTA", fasta_text(lines[0][1:].split()[0], np.frombuffer(b"".join(lines[1:]), np.uint8)))
    with tempfile.TemporaryDirectory() as d:
        gk, rk = synth.CONFIGS["C2"]
        s = synth.make_graph(**gk)
        sb, so, _ = synth.make_reads(s, **rk)
        gfa, rd = os.path.join(d, "c2.gfa"), os.path.join(d, "c2_reads.fa")
        synth.write_gfa(s, gfa)
        synth.write_reads(sb, so, rd)
        args = ["-g", gfa, "-r", rd, "--calls-ref", s.hap_names[0]]
        plain = cli_stages(args + ["-o", os.path.join(d, "c.fa"), "--calls", os.path.join(d, "c.vcf")])
        with open(os.path.join(d, "c.vcf"), "rb") as f:
            add("C2 --calls VCF", f.read())
        if not a.no_cli:
            packed = cli_stages(args + ["--bgzf", "-o", os.path.join(d, "z.fa.gz"), "--calls", os.path.join(d, "z.vcf.gz")])
            for plain_name, packed_name in (("c.fa", "z.fa.gz"), ("c.vcf", "z.vcf.gz")):
                with open(os.path.join(d, plain_name), "rb") as f, gzip.open(os.path.join(d, packed_name), "rb") as z:
                    assert f.read() == z.read(), plain_name
            out["cli_C2"] = {"plain": plain, "bgzf": packed}
            print(json.dumps(out["cli_C2"]), flush=True)
    if not a.no_large:
        g = synth.NativeGraph(backbone_len=174_000_000, n_walks=2, seed=20001)
        seq = np.array(g.seq_concat[:173_800_000])
        g.close()
        add("synthetic FASTA, %d bases" % len(seq), fasta_text(b"synthetic", seq))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
