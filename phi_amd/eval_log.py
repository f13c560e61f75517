#!/usr/bin/env python3
"""eval_log -- the fields the reference's evaluation harness scrapes from a PHI log.

data/postprocessing_2_MIQP.py:55-79 reads, per (sample, coverage) run, `Recombination count`, `Real time`, `Peak RSS`,
`Indexed reads with spectrum size`, `% Minimizers are in ILP` and `Filtered/Retained Minimizers` out of the stderr log
with the regular expressions below, and the edit distance of the output FASTA to a ground truth with edlib.  The log
lines of phi_amd/PHI keep those formats (phi_main.cpp); this module is the same scrape as a function and a small
command line, so that the harness' tables can be made from runs of this build:

    python -m phi_amd.eval_log run1.log [run2.log ...]            # CSV on stdout
    python -m phi_amd.eval_log --truth truth.fa --query out.fa run.log   # + edit distance (banded, exact within the band)
    python -m phi_amd.eval_log --truth truth.fa --query out.fa --identity run.log   # + alignment identity (%.2f)

The edit distance runs on the GPU (phi_edit_distances: whole MHCs in about a second) when a HIP device is present and
libphi_amd.so loads; otherwise on the numpy function below, which is exact but only practical up to some 10^4 bases.
The alignment identity (data/edlib_edits.py: M * 100 / alignment length, of one optimal alignment of the truth as query
against the PHI output as target) likewise comes from phi_edit_alignments, or from the numpy traceback `alignment`.
"""
import argparse
import csv
import re
import sys

# the expressions of data/postprocessing_2_MIQP.py:56, :60, :63, :70, :73, :77
PATTERNS = {
    "recombination_count": (r"Recombination count:\s+(\d+)", int),
    "real_time_s": (r"Real time:\s+(\d+\.\d+)\s+sec", float),
    "peak_rss_gb": (r"Peak RSS:\s+(\d+\.\d+)\s+GB", float),
    "spectrum_size": (r"Indexed reads with spectrum size:\s+(\d+)", int),
    "pct_minimizers_in_ilp": (r"(\d+\.\d+)% Minimizers are in ILP", float),
}
FILTERED = r"Filtered/Retained Minimizers:\s+(\d+\.\d+)/(\d+\.\d+)%"
FIELDS = list(PATTERNS) + ["pct_filtered", "pct_retained"]


def parse_log(text):
    """-> dict of the scraped fields (None where a line is missing, as the harness does)."""
    out = {}
    for key, (pat, conv) in PATTERNS.items():
        m = re.search(pat, text)
        out[key] = conv(m.group(1)) if m else None
    m = re.search(FILTERED, text)
    out["pct_filtered"] = float(m.group(1)) if m else None
    out["pct_retained"] = float(m.group(2)) if m else None
    return out


def read_fasta(path):
    import gzip
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "rb") as f:
        return b"".join(l.strip() for l in f if not l.startswith(b">")).upper()


def edit_distance(a, b, band=None):
    """Global (NW, unit costs) edit distance of two byte strings within a diagonal band: what edlib's NW mode returns
    when the true distance fits the band (the band doubles until it does).  O(len * band) time, numpy rows."""
    import numpy as np
    if len(a) < len(b):
        a, b = b, a
    n, m = len(a), len(b)
    band = band or max(64, (n - m) * 2 + 64)
    A, B = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    while True:
        INF = 1 << 40
        w = 2 * band + 1
        prev = np.full(w, INF, np.int64)
        # row 0: D[0][j] = j for j in [0, band]
        prev[band:band + min(band, m) + 1] = np.arange(0, min(band, m) + 1)
        for i in range(1, n + 1):
            lo = i - band                                          # column of slot 0
            j = np.arange(lo, lo + w)
            valid = (j >= 0) & (j <= m)
            cur = np.full(w, INF, np.int64)
            # substitution / match: D[i-1][j-1] is slot s of prev (the band moves right by one per row)
            jj = np.clip(j - 1, 0, m - 1)
            sub = prev + (A[i - 1] != B[jj])
            sub[j < 1] = INF
            dele = np.concatenate((prev[1:], [INF])) + 1            # D[i-1][j]
            cur = np.minimum(sub, dele)
            cur[j == 0] = i
            cur[~valid] = INF
            # insertions along the row: D[i][j-1] + 1 (prefix minimum of cur[s] - s)
            base = cur - np.arange(w)
            cur = np.minimum(cur, np.minimum.accumulate(base) + np.arange(w))
            cur[~valid] = INF
            prev = cur
        d = int(prev[m - (n - band)]) if 0 <= m - (n - band) < w else INF
        if d <= band - (n - m) or band >= n:
            return d
        band *= 2


def alignment(a, b):
    """One optimal global alignment (unit costs) of query a against target b, by the rule of phi_edit_alignments: from
    (|a|, |b|) back, at each cell the first step that keeps the optimal value -- diagonal, then I (a byte of a only), then
    D (a byte of b only).  -> (M, X, I, D, extended CIGAR).  The DP runs in Ukkonen's band for k = the distance (where it
    is exact on every optimal path), numpy rows; the traceback is a Python loop.  Only practical for small inputs."""
    import numpy as np
    la, lb = len(a), len(b)
    if la == 0 or lb == 0:
        return 0, 0, la, lb, (f"{la}I" if la else "") + (f"{lb}D" if lb else "")
    d = edit_distance(a, b)
    delta = lb - la
    e = (d - abs(delta)) // 2
    xlo, xhi = max(-la, min(0, delta) - e), min(lb, max(0, delta) + e)        # diagonals j - i kept
    w = xhi - xlo + 1
    INF = 1 << 40
    A, B = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    H = np.full((la + 1, w), INF, np.int64)                  # H[i, s]: row i, column i + xlo + s
    s = np.arange(w)
    j0 = xlo + s
    H[0, (j0 >= 0) & (j0 <= lb)] = j0[(j0 >= 0) & (j0 <= lb)]
    for i in range(1, la + 1):
        j = i + xlo + s
        ok = (j >= 0) & (j <= lb)
        prev = H[i - 1]
        dg = prev + (A[i - 1] != B[np.clip(j - 1, 0, lb - 1)])
        dg[j < 1] = INF
        up = np.concatenate((prev[1:], [INF])) + 1
        cur = np.minimum(dg, up)
        cur[j == 0] = i
        cur[~ok] = INF
        cur = np.minimum(cur, np.minimum.accumulate(cur - s) + s)       # + runs along the row
        cur[~ok] = INF
        H[i] = cur
    i, j = la, lb
    v = int(H[i, j - i - xlo])
    assert v == d, (v, d)
    ops = []
    while i > 0 or j > 0:
        k = j - i - xlo
        if i == 0:
            ops.append("D"); j -= 1
        elif j == 0:
            ops.append("I"); i -= 1
        elif H[i - 1, k] + (a[i - 1] != b[j - 1]) == v:
            ops.append("X" if a[i - 1] != b[j - 1] else "="); i -= 1; j -= 1
        elif k + 1 < w and H[i - 1, k + 1] + 1 == v:
            ops.append("I"); i -= 1
        else:
            assert k >= 1 and H[i, k - 1] + 1 == v
            ops.append("D"); j -= 1
        v = int(H[i, j - i - xlo])
    ops.reverse()
    cigar, r = [], 0
    while r < len(ops):
        q = r
        while q < len(ops) and ops[q] == ops[r]:
            q += 1
        cigar.append(f"{q - r}{ops[r]}")
        r = q
    return ops.count("="), ops.count("X"), ops.count("I"), ops.count("D"), "".join(cigar)


def identity(m, x, i, d):
    """data/edlib_edits.py's alignment identity: (alignment length - distance) * 100 / alignment length, 0 when empty"""
    n = m + x + i + d
    return m * 100 / n if n > 0 else 0


def _device_context():
    """A context on device 0, or None when there is no HIP device or the library does not load."""
    try:
        from .context import Context
        return Context(0)
    except (OSError, RuntimeError):
        return None


def main(argv=None):
    ap = argparse.ArgumentParser(description="Scrape PHI logs as data/postprocessing_2_MIQP.py does")
    ap.add_argument("logs", nargs="+")
    ap.add_argument("--truth", help="ground-truth FASTA (with --query: adds the edit distance)")
    ap.add_argument("--query", help="FASTA written by PHI")
    ap.add_argument("--identity", action="store_true",
                    help="with --truth/--query: adds the alignment identity (%%.2f, as data/edlib_edits.py prints it)")
    args = ap.parse_args(argv)
    w = csv.writer(sys.stdout)
    extra = ["edit_distance"] if args.truth and args.query else []
    if extra and args.identity:
        extra.append("alignment_identity")
    w.writerow(["log"] + FIELDS + extra)
    dist = ident = None
    if extra:
        truth, query = read_fasta(args.truth), read_fasta(args.query)
        ctx = _device_context()
        if ctx is not None:
            dist = int(ctx.edit_distances([truth], [query])[0])
            if args.identity:
                al = ctx.edit_alignments([truth], [query], dist=[dist], cigar=False)
                ident = identity(*(int(x) for x in al.counts[0]))
            ctx.close()
        else:
            dist = edit_distance(truth, query)
            if args.identity:
                ident = identity(*alignment(truth, query)[:4])
    for p in args.logs:
        row = parse_log(open(p, errors="replace").read())
        vals = [row[k] for k in FIELDS]
        if extra:
            vals.append(dist)
        if ident is not None:
            vals.append(f"{ident:.2f}")
        w.writerow([p] + vals)


if __name__ == "__main__":
    main()
