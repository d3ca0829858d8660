/* pcm_trace_main.c — the driver of tests/test_pcm_host_trace.py: a fixed list of calls of pcm_host.c's gathered entries (the decimator
 * batch / clips body, the biquad batch, clips and filter-clips entries, the ingest batch) over the stub runtime (pcm_stub_rt.c), the
 * smallest shapes that reach each branch.  The callers' "device" buffers are fixed fake addresses; planar bases sit one sample behind
 * a 16-byte boundary.  After each case: the return value, artamdErrorCount () and the last error text. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "art_internal.h"
#include "decimator.h"

extern int stub_quiet, stub_shards, stub_digest;
void stub_fail (const char *fn, int at);

#define MAXN 16
#define BUF(n)   ((uintptr_t) 0x200000000000 + (uintptr_t)(n) * 0x100000)      /* the callers' buffers, 1 MiB apart */
#define STREAM2  ((void *)(uintptr_t) 0x2f0000000020)
#define COUNTS   ((unsigned long long *) BUF (60))
enum { HERE, ELSEWHERE, SHARDED };                   /* on the lead's stream; on another stream; spread over two devices */
enum { QUICK, SLOW };                                /* a bank that forgets within the warm-up bound (time-parallel), one that never does */

static void begin (const char *name) { printf ("== %s\n", name); }
static void end (int rc)
{
    const char *e = artamdLastError ();
    printf ("-> rc %d errors %d last '%s'\n", rc, artamdErrorCount (), e ? e : "");
    stub_fail (NULL, 0);
}
static void die (const char *what) { fprintf (stderr, "pcm_trace_main: %s\n", what); exit (2); }

/* ---- decimator ---- */
typedef struct { int C, flags, frames, in_planar, out_planar, where; } DecItem;

/* the call `repeat` times over (the second shows what the first left on the host side: swapped generators, fresh mirrors);
 * dup: the last item names the first one's context; fail_fn: that stub's fail_at-th call fails */
static void dec_case (const char *name, const DecItem *items, int n, int lanes, int fromStart, int counts, int repeat, int dup,
                      const char *fail_fn, int fail_at)
{
    Decimate *own [MAXN], *cxts [MAXN];
    const artsample_t *ins [MAXN];
    unsigned char *outs [MAXN];
    long ip [MAXN], op [MAXN];
    int frames [MAXN], in_planes = 0, out_planes = 0;

    stub_quiet = 1;
    for (int i = 0; i < n; ++i) {
        const DecItem *it = &items [i];
        const int bytes = 1 + i % 3;
        stub_shards = it->where == SHARDED ? 2 : 0;
        own [i] = cxts [i] = decimateInit (it->C, 8 * bytes, bytes, 1.0, 44100, it->flags | (it->where == SHARDED ? DECIMATE_MULTITHREADED : 0));
        if (!own [i]) die ("decimateInit failed");
        if (it->where == ELSEWHERE) decimateHipSetStream (own [i], STREAM2);
        frames [i] = it->frames;
        ins [i] = (const artsample_t *)(BUF (2 * i) + (it->in_planar ? sizeof (art_s) : 0));
        outs [i] = (unsigned char *)(BUF (2 * i + 1) + (it->out_planar ? 3 : 0));
        ip [i] = it->in_planar ? it->frames + 5 : 0;
        op [i] = it->out_planar ? (long)(it->frames + 1) * bytes : 0;
        in_planes |= it->in_planar; out_planes |= it->out_planar;
    }
    if (dup) cxts [n - 1] = cxts [0];
    stub_quiet = 0;
    begin (name);
    for (int r = 0; r < repeat; ++r) {
        if (fail_fn) stub_fail (fail_fn, fail_at);
        end (artamd_decimate_clips_planar (cxts, n, ins, in_planes ? ip : NULL, frames, outs, out_planes ? op : NULL, lanes, fromStart, counts ? COUNTS : NULL));
        for (int i = 0; i < n && repeat > 1; ++i)
            printf ("   context %d generator %08x shaper index %d\n", i, own [i]->tpdf_generators ? (unsigned) own [i]->tpdf_generators [0] : 0u,
                    own [i]->noise_shapers ? own [i]->noise_shapers [0].index : -1);
    }
    stub_quiet = 1;
    for (int i = 0; i < n; ++i) decimateFree (own [i]);
    stub_quiet = 0;
}

/* ---- biquad ---- */
typedef struct { int C, S, frames, planar, kind, where; } BqItem;
enum { BATCH, CLIPS, FILTER };
enum { PLAIN, OVERLAP, SHORT_PITCH, MIXED_LAYOUTS, NULL_BUFFER };      /* what is wrong with item 1 of a filter-clips call */

static BiquadBank *make_bank (const BqItem *it)
{
    Biquad sections [16];
    BiquadCoefficients co;
    biquad_lowpass (&co, it->kind == SLOW ? 0.0005 : 0.25);
    for (int k = 0; k < it->C * it->S; ++k) biquad_init (&sections [k], &co, 1.0);
    stub_shards = it->where == SHARDED ? 2 : 0;
    BiquadBank *b = it->where == SHARDED ? biquadBankCreateMulti (sections, it->C, it->S) : biquadBankCreate (sections, it->C, it->S);
    if (!b) die ("biquadBankCreate failed");
    if (it->where == ELSEWHERE) biquadBankSetStream (b, STREAM2);
    return b;
}

/* entry BATCH: a = lanes, b = serialMax; CLIPS: a = fromStart, b = roundBytes in samples; FILTER: a = reversed, b = roundBytes in bytes */
static void bq_case (const char *name, int entry, const BqItem *items, int n, int a, long b, int twist, int dup, const char *fail_fn, int fail_at)
{
    BiquadBank *own [MAXN], *banks [MAXN];
    artsample_t *bufs [MAXN], *outs [MAXN];
    long pitches [MAXN], out_pitches [MAXN];
    int frames [MAXN], planes = 0, rc;

    stub_quiet = 1;
    for (int i = 0; i < n; ++i) {
        const BqItem *it = &items [i];
        own [i] = banks [i] = make_bank (it);
        frames [i] = it->frames;
        bufs [i] = (artsample_t *)(BUF (2 * i) + (it->planar ? sizeof (art_s) : 0));
        outs [i] = (artsample_t *)(BUF (2 * i + 1) + (it->planar ? sizeof (art_s) : 0));
        pitches [i] = out_pitches [i] = it->planar ? it->frames + 3 : 0;
        planes |= it->planar;
    }
    if (dup) banks [n - 1] = banks [0];
    if (twist == OVERLAP) outs [1] = bufs [1] + frames [1] / 2;
    if (twist == SHORT_PITCH) pitches [1] = frames [1] - 1;
    if (twist == MIXED_LAYOUTS) out_pitches [1] = 0;
    if (twist == NULL_BUFFER) outs [1] = NULL;
    stub_quiet = 0;
    begin (name);
    if (fail_fn) stub_fail (fail_fn, fail_at);
    if (entry == BATCH) rc = artamd_biquad_batch_planar (banks, n, bufs, planes ? pitches : NULL, frames, a, (int) b);
    else if (entry == CLIPS) rc = artamd_biquad_clips_planar (banks, n, bufs, planes ? pitches : NULL, frames, a, b * (long) sizeof (art_s));
    else rc = artamd_biquad_filter_clips_planar (banks, n, (const artsample_t *const *) bufs, planes ? pitches : NULL, outs, planes ? out_pitches : NULL, frames, a, b);
    end (rc);
    stub_quiet = 1;
    for (int i = 0; i < n; ++i) biquadBankFree (own [i]);
    stub_quiet = 0;
}

/* ---- ingest ---- */
static void ingest_case (const char *name, int first, int n, int null_at, const char *fail_fn)
{
    const unsigned char *ins [4] = { (const unsigned char *) BUF (0), (const unsigned char *) BUF (2), (const unsigned char *) BUF (4), (const unsigned char *) BUF (6) };
    artsample_t *outs [4] = { (artsample_t *) BUF (1), (artsample_t *) BUF (3), (artsample_t *) BUF (5), (artsample_t *)(BUF (7) + sizeof (art_s)) };
    const double gains [4] = { 1.0, 0.5, 2.0, 0.25 };
    const int bits [4] = { 16, 32, 8, 24 }, bytes [4] = { 2, 4, 1, 3 }, strides [4] = { 1, 1, 2, 3 }, counts [4] = { 100, 50, 0, 37 };
    if (null_at >= 0) outs [null_at] = NULL;
    begin (name);
    if (fail_fn) stub_fail (fail_fn, 1);
    end (floatIntegersBatchLEDevice (ins + first, gains + first, bits + first, bytes + first, strides + first, outs + first, counts + first, n, STREAM2));
}

#define N(list) ((int)(sizeof (list) / sizeof ((list) [0])))
#define ATH SHAPING_ATH_CURVE

int main (void)
{
    /* every class and every side route: the two time-parallel classes, serial lanes of orders 0, 1, 2 (the third-order shaper's filter) and
     * 4 with and without dither, 1 - 3 channels, 0 / 63 / 64 / 100 frames, planar on either side or both */
    static const DecItem dec_all [] = {
        { 2, 0, 100, 0, 0, HERE },
        { 1, DITHER_FLAT, 64, 0, 0, HERE },
        { 3, DITHER_FLAT | SHAPING_1ST_ORDER, 100, 1, 1, HERE },
        { 1, SHAPING_3RD_ORDER, 63, 0, 0, HERE },
        { 1, 0, 63, 0, 0, HERE },
        { 2, DITHER_LOWPASS, 100, 1, 0, HERE },
        { 1, DITHER_FLAT, 0, 0, 0, HERE },
        { 2, DITHER_HIGHPASS | ATH, 64, 0, 1, HERE },
        { 2, DITHER_FLAT, 100, 0, 0, ELSEWHERE },
        { 2, DITHER_FLAT, 100, 1, 1, SHARDED },
    };
    /* the clips forms: a time-parallel item, serial lanes, a context without frames (put back by the grouped copy), two on the side */
    static const DecItem dec_clips [] = {
        { 1, DITHER_FLAT, 64, 0, 0, HERE },
        { 2, DITHER_FLAT | SHAPING_1ST_ORDER, 100, 1, 1, HERE },
        { 1, DITHER_FLAT | SHAPING_2ND_ORDER, 0, 0, 0, HERE },
        { 2, DITHER_FLAT, 100, 0, 0, ELSEWHERE },
        { 2, 0, 0, 0, 0, ELSEWHERE },
    };
    static const DecItem dec_serial [] = { { 3, DITHER_FLAT | SHAPING_1ST_ORDER, 100, 1, 1, HERE }, { 1, 0, 63, 0, 0, HERE } };
    static const DecItem dec_empty [] = { { 2, DITHER_FLAT, 0, 0, 0, HERE }, { 1, 0, 0, 0, 0, HERE } };
    static const DecItem dec_small [] = { { 1, DITHER_FLAT, 100, 0, 0, HERE }, { 1, DITHER_FLAT | ATH, 64, 0, 0, HERE }, { 1, DITHER_FLAT, 0, 0, 0, HERE } };

    stub_digest = 0;
    dec_case ("decimate batch", dec_all, N (dec_all), 0, 0, 0, 1, 0, NULL, 0);
    stub_digest = 1;
    dec_case ("decimate batch twice", dec_small, N (dec_small), 0, 0, 0, 2, 0, NULL, 0);
    stub_digest = 0;
    dec_case ("decimate clips fromStart", dec_clips, N (dec_clips), 0, 1, 0, 1, 0, NULL, 0);
    stub_digest = 1;
    dec_case ("decimate clips fromStart twice", dec_small, N (dec_small), 0, 1, 0, 2, 0, NULL, 0);
    stub_digest = 0;
    dec_case ("decimate clips counts", dec_clips, N (dec_clips), 0, 0, 1, 1, 0, NULL, 0);
    stub_digest = 1;
    dec_case ("decimate clips fromStart counts", dec_small, N (dec_small), 0, 1, 1, 1, 0, NULL, 0);
    stub_digest = 0;
    dec_case ("decimate batch lanes 2", dec_serial, N (dec_serial), 2, 0, 0, 1, 0, NULL, 0);
    stub_digest = 1;
    dec_case ("decimate batch lanes 70", dec_serial + 1, 1, 70, 0, 0, 1, 0, NULL, 0);
    dec_case ("decimate batch n 0", dec_small, 0, 0, 0, 0, 1, 0, NULL, 0);
    dec_case ("decimate batch nothing to do", dec_empty, N (dec_empty), 0, 0, 0, 1, 0, NULL, 0);
    dec_case ("decimate clips only restores", dec_empty, N (dec_empty), 0, 1, 0, 1, 0, NULL, 0);
    dec_case ("decimate batch duplicate", dec_small, N (dec_small), 0, 0, 0, 1, 1, NULL, 0);
    dec_case ("decimate batch upload fails", dec_small, N (dec_small), 0, 0, 0, 1, 0, "arthip_table_upload", 1);
    dec_case ("decimate batch grow fails", dec_small, N (dec_small), 0, 0, 0, 1, 0, "arthip_grow", 1);
    dec_case ("decimate batch launch fails", dec_small, N (dec_small), 0, 0, 0, 1, 0, "arthip_decimate_batch_launch", 1);
    dec_case ("decimate clips second launch fails", dec_small, N (dec_small), 0, 1, 1, 1, 0, "arthip_decimate_batch_launch", 2);
    dec_case ("decimate clips restore launch fails", dec_small, N (dec_small), 0, 1, 0, 1, 0, "arthip_copy_rows_launch", 1);
    dec_case ("decimate clips counts not cleared", dec_small, N (dec_small), 0, 0, 1, 1, 0, "arthip_zero", 1);
    dec_case ("decimate clips count upload fails", dec_clips + 2, 2, 0, 0, 1, 1, 0, "arthip_h2d", 1);

    /* S = 1 .. 4; a time-parallel bank at 512 frames (gathered) and at 600 (the side call), in both layouts; a planar serial item;
     * an empty one; a bank on another stream and a sharded one */
    static const BqItem bq_all [] = {
        { 2, 1, 512, 0, QUICK, HERE },
        { 1, 1, 600, 0, QUICK, HERE },
        { 3, 2, 100, 1, SLOW, HERE },
        { 1, 3, 50, 1, SLOW, HERE },
        { 1, 4, 10, 0, SLOW, HERE },
        { 2, 1, 0, 0, SLOW, HERE },
        { 2, 1, 600, 1, QUICK, HERE },
        { 2, 2, 100, 0, SLOW, ELSEWHERE },
        { 2, 2, 100, 1, SLOW, SHARDED },
    };
    static const BqItem bq_small [] = { { 3, 2, 100, 1, SLOW, HERE }, { 1, 1, 512, 0, QUICK, HERE }, { 1, 2, 7, 0, SLOW, HERE } };
    static const BqItem bq_sides [] = { { 1, 1, 600, 0, QUICK, HERE }, { 2, 1, 0, 0, SLOW, HERE } };

    stub_digest = 0;
    bq_case ("biquad batch", BATCH, bq_all, N (bq_all), 0, -1, PLAIN, 0, NULL, 0);
    stub_digest = 1;
    bq_case ("biquad batch serialMax 0", BATCH, bq_small, N (bq_small), 0, 0, PLAIN, 0, NULL, 0);
    stub_digest = 0;
    bq_case ("biquad batch lanes 2", BATCH, bq_small, N (bq_small), 2, -1, PLAIN, 0, NULL, 0);
    stub_digest = 1;
    bq_case ("biquad batch lanes 70", BATCH, bq_small + 1, 1, 70, -1, PLAIN, 0, NULL, 0);
    bq_case ("biquad batch interleaved only", BATCH, bq_small + 1, 2, 0, -1, PLAIN, 0, NULL, 0);
    bq_case ("biquad batch n 0", BATCH, bq_small, 0, 0, -1, PLAIN, 0, NULL, 0);
    bq_case ("biquad batch only side calls", BATCH, bq_sides, N (bq_sides), 0, -1, PLAIN, 0, NULL, 0);
    bq_case ("biquad batch duplicate", BATCH, bq_small, N (bq_small), 0, -1, PLAIN, 1, NULL, 0);
    bq_case ("biquad batch upload fails", BATCH, bq_small + 1, 2, 0, -1, PLAIN, 0, "arthip_table_upload", 1);
    bq_case ("biquad batch grow fails", BATCH, bq_small + 1, 2, 0, -1, PLAIN, 0, "arthip_grow", 1);
    bq_case ("biquad batch second launch fails", BATCH, bq_small + 1, 2, 0, -1, PLAIN, 0, "arthip_biquad_batch_launch", 2);

    /* three gathered items in both layouts and two section counts, a serial item, an empty one, a side bank */
    static const BqItem clips_all [] = {
        { 2, 1, 600, 0, QUICK, HERE },
        { 2, 1, 700, 1, QUICK, HERE },
        { 3, 2, 100, 1, SLOW, HERE },
        { 1, 2, 1300, 0, QUICK, HERE },
        { 2, 1, 0, 0, QUICK, HERE },
        { 2, 1, 600, 0, QUICK, ELSEWHERE },
        { 2, 1, 0, 0, QUICK, ELSEWHERE },
    };
    static const BqItem clips_fail [] = { { 1, 1, 600, 0, QUICK, HERE }, { 1, 1, 700, 0, QUICK, HERE }, { 1, 2, 100, 0, SLOW, HERE } };
    static const BqItem clips_lone [] = { { 2, 1, 600, 1, QUICK, HERE }, { 1, 2, 100, 0, SLOW, HERE }, { 2, 1, 0, 0, SLOW, HERE } };
    static const BqItem clips_small [] = { { 1, 1, 600, 0, QUICK, HERE }, { 2, 1, 700, 1, QUICK, HERE }, { 1, 2, 100, 0, SLOW, HERE } };
    static const BqItem clips_serial [] = { { 1, 2, 100, 0, SLOW, HERE }, { 1, 1, 40, 1, SLOW, HERE } };

    stub_digest = 0;
    bq_case ("biquad clips", CLIPS, clips_small, N (clips_small), 0, 0, PLAIN, 0, NULL, 0);
    bq_case ("biquad clips fromStart three rounds", CLIPS, clips_all, N (clips_all), 1, 2600, PLAIN, 0, NULL, 0);
    stub_digest = 1;
    bq_case ("biquad clips every item beyond the bound", CLIPS, clips_fail, 2, 0, 100, PLAIN, 0, NULL, 0);
    bq_case ("biquad clips lone gathered item", CLIPS, clips_lone, N (clips_lone), 0, 0, PLAIN, 0, NULL, 0);
    bq_case ("biquad clips lone gathered item fromStart", CLIPS, clips_lone, N (clips_lone), 1, 0, PLAIN, 0, NULL, 0);
    bq_case ("biquad clips serial only", CLIPS, clips_serial, N (clips_serial), 0, 0, PLAIN, 0, NULL, 0);
    bq_case ("biquad clips serial only fromStart", CLIPS, clips_serial, N (clips_serial), 1, 0, PLAIN, 0, NULL, 0);
    bq_case ("biquad clips nothing to do", CLIPS, clips_lone + 2, 1, 0, 0, PLAIN, 0, NULL, 0);
    bq_case ("biquad clips n 0", CLIPS, clips_small, 0, 0, 0, PLAIN, 0, NULL, 0);
    bq_case ("biquad clips duplicate", CLIPS, clips_small, N (clips_small), 0, 0, PLAIN, 1, NULL, 0);
    bq_case ("biquad clips upload fails", CLIPS, clips_fail, N (clips_fail), 1, 0, PLAIN, 0, "arthip_table_upload", 1);
    bq_case ("biquad clips scratch grow fails", CLIPS, clips_fail, N (clips_fail), 1, 0, PLAIN, 0, "arthip_grow", 2);
    bq_case ("biquad clips copy launch fails", CLIPS, clips_fail, N (clips_fail), 1, 0, PLAIN, 0, "arthip_copy_rows_launch", 1);
    bq_case ("biquad clips class launch fails", CLIPS, clips_fail, N (clips_fail), 1, 0, PLAIN, 0, "arthip_biquad_clips_launch", 1);
    bq_case ("biquad clips batch part fails", CLIPS, clips_fail, N (clips_fail), 1, 0, PLAIN, 0, "arthip_biquad_batch_launch", 1);

    /* the same routes out of place; the serial class of S = 2 has 3 + 2 lanes (padded), a bank on another stream is only read */
    static const BqItem filter_all [] = {
        { 2, 1, 600, 0, QUICK, HERE },
        { 2, 1, 700, 1, QUICK, HERE },
        { 3, 2, 100, 1, SLOW, HERE },
        { 1, 2, 1300, 0, QUICK, HERE },
        { 2, 1, 0, 0, QUICK, HERE },
        { 2, 2, 100, 0, SLOW, ELSEWHERE },
        { 1, 4, 40, 0, QUICK, HERE },
    };
    static const BqItem filter_sharded_lead [] = { { 2, 1, 600, 0, QUICK, SHARDED }, { 2, 1, 600, 0, QUICK, HERE } };
    static const BqItem filter_sharded_item [] = { { 2, 1, 600, 0, QUICK, HERE }, { 2, 1, 600, 0, QUICK, SHARDED } };
    static const BqItem filter_planar [] = { { 2, 1, 600, 1, QUICK, HERE }, { 3, 1, 100, 1, SLOW, HERE } };

    stub_digest = 0;
    bq_case ("filter clips forwards", FILTER, filter_planar, N (filter_planar), 0, 0, PLAIN, 0, NULL, 0);
    bq_case ("filter clips reversed three rounds", FILTER, filter_all, N (filter_all), 1, 256, PLAIN, 0, NULL, 0);
    bq_case ("filter clips serial only", FILTER, clips_serial, N (clips_serial), 0, 0, PLAIN, 0, NULL, 0);
    stub_digest = 1;
    bq_case ("filter clips gathered only", FILTER, clips_fail, 2, 1, 0, PLAIN, 0, NULL, 0);
    bq_case ("filter clips nothing to do", FILTER, clips_lone + 2, 1, 0, 0, PLAIN, 0, NULL, 0);
    bq_case ("filter clips n 0", FILTER, filter_planar, 0, 0, 0, PLAIN, 0, NULL, 0);
    bq_case ("filter clips refuses overlap", FILTER, filter_planar, N (filter_planar), 0, 0, OVERLAP, 0, NULL, 0);
    bq_case ("filter clips refuses a pitch below the frames", FILTER, filter_planar, N (filter_planar), 0, 0, SHORT_PITCH, 0, NULL, 0);
    bq_case ("filter clips refuses mixed layouts", FILTER, filter_planar, N (filter_planar), 0, 0, MIXED_LAYOUTS, 0, NULL, 0);
    bq_case ("filter clips refuses a NULL buffer", FILTER, filter_planar, N (filter_planar), 0, 0, NULL_BUFFER, 0, NULL, 0);
    bq_case ("filter clips refuses a sharded lead", FILTER, filter_sharded_lead, N (filter_sharded_lead), 0, 0, PLAIN, 0, NULL, 0);
    bq_case ("filter clips refuses a sharded item", FILTER, filter_sharded_item, N (filter_sharded_item), 0, 0, PLAIN, 0, NULL, 0);
    bq_case ("filter clips duplicate", FILTER, filter_planar, N (filter_planar), 0, 0, PLAIN, 1, NULL, 0);
    bq_case ("filter clips upload fails", FILTER, filter_planar, N (filter_planar), 0, 0, PLAIN, 0, "arthip_table_upload", 1);
    bq_case ("filter clips grow fails", FILTER, filter_planar, N (filter_planar), 0, 0, PLAIN, 0, "arthip_grow", 2);
    bq_case ("filter clips serial launch fails", FILTER, filter_planar, N (filter_planar), 0, 0, PLAIN, 0, "arthip_biquad_filter_batch_launch", 1);
    bq_case ("filter clips class launch fails", FILTER, clips_fail, 2, 1, 0, PLAIN, 0, "arthip_biquad_filter_clips_launch", 1);

    /* items 1 (more than 24 bits) and 2 (no samples) are skipped; item 3's output sits one sample behind a 16-byte boundary */
    ingest_case ("ingest batch", 0, 4, -1, NULL);
    ingest_case ("ingest batch all skipped", 1, 2, -1, NULL);
    ingest_case ("ingest batch NULL buffer of a skipped item", 0, 4, 1, NULL);
    ingest_case ("ingest batch NULL buffer", 0, 4, 3, NULL);
    ingest_case ("ingest batch n 0", 0, 0, -1, NULL);
    ingest_case ("ingest batch launch fails", 0, 4, -1, "arthip_ingest_batch");
    return 0;
}
