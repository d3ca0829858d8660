/* extrapolate_host.c — host glue of the device LPC extrapolation (artamdExtrapolateBatchDevice): argument checks and the run
 * table.  The fit and the prediction run on the device (extrapolate_kernels.hip); there is no host implementation. */
#include <stdio.h>
#include <stdlib.h>

#include "art_internal.h"

int artamdExtrapolateBatchDevice (const artsample_t *const *d_known, const int *counts, const int *strides, const int *backward,
                                  artsample_t *const *d_out, const int *extras, int n, void *hipStream)
{
    int live = 0;
    if (n <= 0) return 0;
    if (!d_known || !counts || !strides || !backward || !d_out || !extras) {
        fprintf (stderr, "artamd: extrapolate batch: a NULL argument array\n");
        return -1;
    }
    for (int i = 0; i < n; ++i) {
        if (counts [i] < 8 || counts [i] > ARTAMD_EXTRAPOLATE_MAX_KNOWN || extras [i] < 0 || strides [i] < 1) {
            fprintf (stderr, "artamd: extrapolate batch: run %d: count %d (8 .. %d), extras %d (>= 0), stride %d (>= 1)\n",
                     i, counts [i], ARTAMD_EXTRAPOLATE_MAX_KNOWN, extras [i], strides [i]);
            return -1;
        }
        if (!extras [i]) continue;
        if (!d_known [i] || !d_out [i]) { fprintf (stderr, "artamd: extrapolate batch: run %d: a NULL buffer pointer\n", i); return -1; }
        ++live;
    }
    if (!live) return 0;

    ArtExtrapRun *runs = calloc ((size_t) live, sizeof (ArtExtrapRun));
    if (!runs) { artamd_note_failure ("extrapolate batch: out of host memory"); return -1; }
    for (int i = 0, j = 0; i < n; ++i) {
        if (!extras [i]) continue;
        ArtExtrapRun *r = &runs [j++];
        r->src [0] = d_known [i]; r->stride [0] = strides [i]; r->n [0] = counts [i];
        r->src [1] = d_known [i]; r->stride [1] = 1; r->n [1] = 0;
        r->out = d_out [i]; r->out_stride = strides [i];
        r->extras = extras [i]; r->backward = backward [i] != 0;
    }
    const int rc = arthip_extrapolate (runs, live, hipStream);
    free (runs);
    if (rc) { artamd_note_failure ("extrapolate batch: the table could not be uploaded or the launch failed"); return -1; }
    return 0;
}
