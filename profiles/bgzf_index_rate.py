"""The BGZF indexes built on the device (phi_deflate_bgzf_indexed, bgzf_index.hip): what the index costs beside
the file.  Run by hand on the MI355X; writes profiles/bgzf_index_rate.json, everything taken in one run:

  (i)   per text -- the MHC_4 VCF of tests/golden/data (4.9 MB) and that text tiled with shifted POS to at least 64 MB -- the
        device_ms of phi_bgzf_index_info (the index kernels alone), the wall time of phi_amd.deflate_bgzf_indexed (kind "tbi")
        against phi_amd.deflate_bgzf on the same input, both through Python; a warm-up, then --repeats runs, the median
  (ii)  the per-line writer of tests/tabix_ref.py for the same index on one core (once per text; the large text only with
        --reference-large: it takes minutes)
  (iii) the stage "calls (device) + VCF write" of one `PHI --bgzf --calls` command at C2, without and with --bgzf-index

    python profiles/bgzf_index_rate.py [--repeats 3] [--no-large] [--no-cli] [--reference-large] [--out FILE]
"""
import argparse
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401  (its HIP runtime initialises first, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import phi_amd                                                  # noqa: E402
from phi_amd import synth                                       # noqa: E402
import tabix_ref as T                                           # noqa: E402

PHI = os.path.join(ROOT, "phi_amd", "PHI")
DATA = os.path.join(ROOT, "tests", "golden", "data")
STAGE = re.compile(r"\[phi timing\] main: stage (.+?)\s+[\d.]+ ->\s+[\d.]+ s\s+\(\s*([\d.]+) ms\)")


def tiled(text, least):
    """the records of text again and again, POS shifted by the span of the copies before, until the text holds `least` bytes"""
    lines = text.split(b"\n")
    meta = [ln for ln in lines if ln.startswith(b"#")]
    recs = [ln.split(b"\t", 2) for ln in lines if ln and not ln.startswith(b"#")]
    span = max(int(r[1]) for r in recs) + 1000000
    out, size, k = [b"\n".join(meta)], 0, 0
    while size < least:
        part = b"\n".join(b"\t".join((r[0], b"%d" % (int(r[1]) + k * span), r[2])) for r in recs)
        out.append(part)
        size += len(part) + 1
        k += 1
    assert k * span < 1 << 29, "the tiled positions leave the range of a .tbi"
    return b"\n".join(out) + b"\n"


def measure(name, text, repeats, reference):
    row = {"text": name, "bytes": len(text), "runs": []}
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        plain = phi_amd.deflate_bgzf(text)
        t1 = time.perf_counter()
        data, tbi, info = phi_amd.deflate_bgzf_indexed(text, "tbi")
        t2 = time.perf_counter()
        assert data == plain
        if rep:                                                 # (the first turn is the warm-up)
            row["runs"].append({"index_device_ms": info["device_ms"], "deflate_device_ms": info["deflate"]["device_ms"],
                                "plain_wall_ms": (t1 - t0) * 1e3, "indexed_wall_ms": (t2 - t1) * 1e3})
    row.update({k: int(info[k]) for k in ("records", "contigs", "bins", "chunks", "windows", "index_bytes")})
    row["median"] = {k: float(np.median([r[k] for r in row["runs"]])) for k in row["runs"][0]}
    row["median"]["index_gb_per_s"] = len(text) / row["median"]["index_device_ms"] / 1e6
    if reference:
        t0 = time.perf_counter()
        want, _ = T.tbi_bytes(text, T.member_offsets(data))
        row["per_line_writer_one_core_ms"] = (time.perf_counter() - t0) * 1e3
        assert T.inflate_all(tbi) == want
    return row


def cli_stage(args):
    r = subprocess.run([PHI] + args, capture_output=True, text=True, timeout=900, env=dict(os.environ, PHI_TIMING="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    ms = {m.group(1).strip(): float(m.group(2)) for m in STAGE.finditer(r.stderr)}
    return {"fasta_write_ms": ms["FASTA write"], "calls_and_vcf_write_ms": ms["calls (device) + VCF write"],
            "index_lines": [re.sub(r"written to \S*/", "written to ", ln.split("] ", 1)[-1]) for ln in r.stderr.splitlines() if "BGZF index: " in ln]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--reference-large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_index_rate.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "texts": []}

    def add(name, text, reference):
        out["texts"].append(measure(name, text, a.repeats, reference))
        print(json.dumps({k: v for k, v in out["texts"][-1].items() if k != "runs"}), flush=True)

    with gzip.open(os.path.join(DATA, "MHC_4.vcf.gz"), "rb") as f:
        mhc = f.read()
    add("MHC_4 VCF", mhc, True)
    if not a.no_large:
        add("MHC_4 VCF tiled with shifted POS", tiled(mhc, 64 << 20), a.reference_large)
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as d:
            gk, rk = synth.CONFIGS["C2"]
            s = synth.make_graph(**gk)
            sb, so, _ = synth.make_reads(s, **rk)
            gfa, rd = os.path.join(d, "c2.gfa"), os.path.join(d, "c2_reads.fa")
            synth.write_gfa(s, gfa)
            synth.write_reads(sb, so, rd)
            args = ["-g", gfa, "-r", rd, "--calls-ref", s.hap_names[0], "--bgzf"]
            plain = cli_stage(args + ["-o", os.path.join(d, "a.fa.gz"), "--calls", os.path.join(d, "a.vcf.gz")])
            indexed = cli_stage(args + ["--bgzf-index", "-o", os.path.join(d, "b.fa.gz"), "--calls", os.path.join(d, "b.vcf.gz")])
            for n in ("fa.gz", "vcf.gz"):
                with open(os.path.join(d, "a." + n), "rb") as f, open(os.path.join(d, "b." + n), "rb") as g:
                    assert f.read() == g.read(), n
            out["cli_C2"] = {"bgzf": plain, "bgzf_index": indexed}
            print(json.dumps(out["cli_C2"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
