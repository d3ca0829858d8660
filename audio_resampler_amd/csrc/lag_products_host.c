/* lag_products_host.c — host glue of the lagged inner products (artamdLagProductsBatchDevice): the argument checks, which need no
 * device.  The table, the scratch and the launches are lag_products.hip's; there is no host implementation. */
#include <stdio.h>

#include "art_internal.h"

#if ART_LAG_MAX != ARTAMD_LAG_PRODUCTS_MAX
#error "the kernel's lag count and the header's differ"
#endif

/* the tile length in frames (for the tests: a row's sums are its tiles' partials in ascending order) */
int artamd_lag_products_tile (void) { return ART_LAG_TILE; }

int artamdLagProductsBatchDevice (const artsample_t *const *d_u, const artsample_t *const *d_v, const int *numFrames,
                                  const int *firstLags, const int *numLags, double *const *d_sums, int n, void *hipStream)
{
    int live = 0;
    if (n <= 0) return 0;
    if (!d_u || !d_v || !numFrames || !firstLags || !numLags || !d_sums) {
        fprintf (stderr, "artamd: lag products: a NULL argument array\n");
        return -1;
    }
    for (int i = 0; i < n; ++i) {
        if (numFrames [i] <= 0) continue;
        if (!d_u [i] || !d_v [i] || !d_sums [i]) { fprintf (stderr, "artamd: lag products: row %d: a NULL pointer\n", i); return -1; }
        if (firstLags [i] < 0 || numLags [i] < 1 || numLags [i] > ARTAMD_LAG_PRODUCTS_MAX || firstLags [i] > ARTAMD_LAG_PRODUCTS_MAX - numLags [i]) {
            fprintf (stderr, "artamd: lag products: row %d: first lag %d (>= 0), %d lags (>= 1), both within %d\n",
                     i, firstLags [i], numLags [i], ARTAMD_LAG_PRODUCTS_MAX);
            return -1;
        }
        ++live;
    }
    if (!live) return 0;
    const int rc = arthip_lag_products (d_u, d_v, numFrames, firstLags, numLags, d_sums, n, live, hipStream);
    if (rc < 0) { artamd_note_failure ("lag products: out of memory for the table or the partials, or a launch failed"); return -1; }
    return rc;
}
