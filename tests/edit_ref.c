/* Test reference for phi_edit_distances: unit-cost global edit distance by Myers' O(ND) diagonal-transition algorithm
 * (E. W. Myers, "An O(ND) difference algorithm and its variations", Algorithmica 1986), with substitutions as well as
 * indels: for every diagonal k = y - x keep the furthest x reached with at most d edits, then slide along matches.
 * Deliberately not the kernel's algorithm (bit-parallel, banded).  Built by the tests with `cc -O2 -shared` and called
 * through ctypes.
 *
 * ond_edit_distance(a, n, b, m, max_d): the distance, or -1 when it exceeds max_d (max_d < 0: no limit). */
#include <stdint.h>
#include <stdlib.h>

#define BETTER(v) do { if ((v) > best) best = (v); } while (0)

int64_t ond_edit_distance(const uint8_t *a, int64_t n, const uint8_t *b, int64_t m, int64_t max_d)
{
    const int64_t limit = max_d < 0 || max_d > n + m ? n + m : max_d;
    int64_t *cur = (int64_t *)malloc(sizeof(int64_t) * (size_t)(2 * limit + 3));
    int64_t *nxt = (int64_t *)malloc(sizeof(int64_t) * (size_t)(2 * limit + 3));
    int64_t result = -1;
    if (!cur || !nxt) goto done;
    /* cur[k + limit + 1] for k in [-d, d]: furthest x on diagonal k (-1: unreachable) */
    {
        int64_t x = 0;
        while (x < n && x < m && a[x] == b[x]) x++;
        cur[limit + 1] = x;
        if (n == m && x == n) { result = 0; goto done; }
    }
    for (int64_t d = 1; d <= limit; d++) {
        for (int64_t k = -d; k <= d; k++) {
            int64_t best = -1;
            if (k > -d && k < d) {                       /* same diagonal: the old point, or a substitution after it */
                const int64_t x = cur[k + limit + 1];
                if (x >= 0) { BETTER(x); if (x < n && x + k < m) BETTER(x + 1); }
            }
            if (k + 1 <= d - 1) {                        /* from k + 1: a[x] deleted */
                const int64_t x = cur[k + 1 + limit + 1];
                if (x >= 0 && x < n) BETTER(x + 1);
            }
            if (k - 1 >= -(d - 1)) {                     /* from k - 1: b[y] inserted */
                const int64_t x = cur[k - 1 + limit + 1];
                if (x >= 0 && x + k <= m) BETTER(x);
            }
            if (best >= 0) while (best < n && best + k < m && a[best] == b[best + k]) best++;
            nxt[k + limit + 1] = best;
        }
        int64_t *sw = cur; cur = nxt; nxt = sw;
        const int64_t kend = m - n;
        if (kend >= -d && kend <= d && cur[kend + limit + 1] == n) { result = d; goto done; }
    }
done:
    free(cur);
    free(nxt);
    return result;
}
