/* Test reference for phi_edit_alignments: the unit-cost global DP of query a (rows) against target b (columns), and the
 * traceback of the documented rule -- from (|a|, |b|), at each cell the first step that keeps the optimal value: the
 * diagonal ('=' or 'X'), then the step that consumes a only ('I'), then the one that consumes b only ('D').  The whole
 * matrix, or with band >= 0 only the diagonals j - i in [min(0, |b|-|a|) - e, max(0, |b|-|a|) + e], e = (band -
 * ||b|-|a||) / 2 (Ukkonen's band: every path of cost <= band stays in it, and the values there are exact on such paths).
 * One byte per cell holds which predecessors keep the value; two rows of values.  Built by the tests with
 * `cc -O2 -shared` and called through ctypes.
 *
 * ref_align(a, la, b, lb, band, cigar, cap, out): out[0..4] = M, X, I, D, cost; the CIGAR ('=', 'X', 'I', 'D' runs) goes
 * to cigar[0 .. cap).  Returns its length, -1 when the band does not reach (|a|, |b|) or memory is short, -2 when cap is. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define INF ((int64_t)1 << 50)

int64_t ref_align(const uint8_t *a, int64_t la, const uint8_t *b, int64_t lb, int64_t band, char *cigar, int64_t cap, int64_t *out)
{
    int64_t xlo = -la, xhi = lb;                             /* diagonals j - i kept */
    if (band >= 0) {
        const int64_t delta = lb - la, ad = delta < 0 ? -delta : delta;
        if (band < ad) return -1;
        const int64_t e = (band - ad) / 2;
        xlo = (delta < 0 ? delta : 0) - e;
        xhi = (delta > 0 ? delta : 0) + e;
        if (xlo < -la) xlo = -la;
        if (xhi > lb) xhi = lb;
    }
    const int64_t w = xhi - xlo + 1;
    uint8_t *how = (uint8_t *)calloc((size_t)((la + 1) * w), 1);   /* bit 0 diagonal, 1 up (I), 2 left (D) */
    int64_t *prev = (int64_t *)malloc(sizeof(int64_t) * (size_t)(w + 2)), *cur = (int64_t *)malloc(sizeof(int64_t) * (size_t)(w + 2));
    char *ops = (char *)malloc((size_t)(la + lb + 1));
    int64_t ret = -1;
    if (!how || !prev || !cur || !ops) goto done;
    /* row i, column j at slot j - i - xlo + 1 of prev / cur (slots 0 and w + 1 stay INF) */
    for (int64_t i = 0; i <= la; i++) {
        for (int64_t s = 0; s < w + 2; s++) cur[s] = INF;
        for (int64_t j = i + xlo < 0 ? 0 : i + xlo; j <= i + xhi && j <= lb; j++) {
            const int64_t s = j - i - xlo + 1;
            int64_t v;
            uint8_t h = 0;
            if (i == 0) { v = j; h = j ? 4 : 0; }
            else if (j == 0) { v = i; h = 2; }
            else {
                const int64_t dg = prev[s] + (a[i - 1] != b[j - 1]), up = prev[s + 1] + 1, lf = cur[s - 1] + 1;
                v = dg < up ? dg : up;
                if (lf < v) v = lf;
                h = (uint8_t)((dg == v) | (up == v) << 1 | (lf == v) << 2);
            }
            cur[s] = v;
            how[i * w + s - 1] = h;
        }
        int64_t *t = prev; prev = cur; cur = t;
    }
    if (lb - la < xlo || lb - la > xhi) goto done;
    out[4] = prev[lb - la - xlo + 1];
    out[0] = out[1] = out[2] = out[3] = 0;
    int64_t n_ops = 0;
    for (int64_t i = la, j = lb; i > 0 || j > 0;) {
        const uint8_t h = how[i * w + (j - i - xlo)];
        if (h & 1) { const int x = a[i - 1] != b[j - 1]; ops[n_ops++] = x ? 'X' : '='; out[x]++; i--; j--; }
        else if (h & 2) { ops[n_ops++] = 'I'; out[2]++; i--; }
        else if (h & 4) { ops[n_ops++] = 'D'; out[3]++; j--; }
        else goto done;                                     /* (cannot happen: every cell but (0, 0) has a predecessor) */
    }
    ret = 0;
    for (int64_t k = n_ops - 1; k >= 0;) {                 /* ops were collected backwards */
        int64_t r = k;
        while (r >= 0 && ops[r] == ops[k]) r--;
        char tmp[32];
        const int len = snprintf(tmp, sizeof tmp, "%lld%c", (long long)(k - r), ops[k]);
        if (ret + len > cap) { ret = -2; goto done; }
        for (int q = 0; q < len; q++) cigar[ret + q] = tmp[q];
        ret += len;
        k = r;
    }
done:
    free(how); free(prev); free(cur); free(ops);
    return ret;
}
