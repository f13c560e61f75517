#!/usr/bin/env python3
"""edlib_edits -- the command line of the reference's data/edlib_edits.py on this build.

    python -m phi_amd.edlib_edits query.fa reference.fa

reads the first record of each FASTA file (bytes as they are: no case folding) and prints, as the reference does,

    Edit distance: N
    Alignment identity: X.XX%

where identity = (alignment length - distance) * 100 / alignment length of one optimal global alignment of query
against reference (0 when both are empty).  data/postprocessing_2_MIQP.py:21-39 (compute_edlib_metrics) scrapes both
lines.  The distance and the alignment come from phi_edit_distances / phi_edit_alignments when a HIP device is present
and libphi_amd.so loads; otherwise from eval_log's numpy DP and traceback (only practical for small inputs).
"""
import argparse
import gzip

from .eval_log import _device_context, alignment, identity


def read_first_record(path):
    """The sequence of the first FASTA record of path (.gz allowed), its lines joined, bytes unchanged."""
    op = gzip.open if str(path).endswith(".gz") else open
    seq, started = [], False
    with op(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if started:
                    break
                started = True
                continue
            if started:
                seq.append(line.strip())
    return b"".join(seq)


def metrics(query, reference):
    """-> (edit distance, alignment identity in percent) of query against reference."""
    ctx = _device_context()
    if ctx is not None:
        try:
            al = ctx.edit_alignments([query], [reference], cigar=False)
            return int(al.distance[0]), identity(*(int(x) for x in al.counts[0]))
        finally:
            ctx.close()
    m, x, i, d, _ = alignment(query, reference)
    return x + i + d, identity(m, x, i, d)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Compute edit distance and alignment identity between two FASTA sequences.")
    ap.add_argument("query_fasta", help="Path to the query FASTA file")
    ap.add_argument("reference_fasta", help="Path to the reference FASTA file")
    args = ap.parse_args(argv)
    dist, ident = metrics(read_first_record(args.query_fasta), read_first_record(args.reference_fasta))
    print(f"Edit distance: {dist}")
    print(f"Alignment identity: {ident:.2f}%")


if __name__ == "__main__":
    main()
