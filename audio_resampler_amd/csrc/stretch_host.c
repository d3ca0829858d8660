/* stretch_host.c — host side of the time stretcher: the reference's stretch.h API (reference stretch.c:50-143,
 * :335-373 for init / reset / capacity / flush / free; the per-call state machine itself runs on the device,
 * stretch_kernels.hip).  No CPU path: without a HIP device stretchInit fails loudly. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "art_internal.h"
#include "stretch.h"

typedef struct { int mark, fill, cur, pad; double drift; } DevState;   /* must match stretch_kernels.hip */

struct artamd_stretch {
    ArtStretchArgs args;
    art_s *d_in, *d_out; size_t in_cap, out_cap;      /* staging for host-pointer calls (bytes) */
    int *d_result;
    void *stream;
    int blocks;                                        /* ring size in longest periods: 3, or 4 in fast mode */
    void *d_batch; size_t batch_cap;                   /* batched calls led by this context: items + results */
    unsigned long batch_stamp;                         /* last batched call this context took part in (duplicate check) */
};

static int push_state (Stretch *cxt)                   /* host mirrors -> device state (init / reset) */
{
    DevState st [2];
    memset (st, 0, sizeof (st));
    st [0].mark = cxt->tail; st [0].fill = cxt->head; st [0].drift = cxt->outsamples_error;
    if (cxt->next) { st [1].mark = cxt->next->tail; st [1].fill = cxt->next->head; st [1].drift = cxt->next->outsamples_error; }
    return arthip_h2d (cxt->hip->args.state, st, sizeof (st), cxt->hip->stream) || arthip_sync (cxt->hip->stream);
}

static void pull_state (Stretch *cxt)                  /* device state -> host mirrors (after every call) */
{
    DevState st [2];
    if (arthip_d2h (st, cxt->hip->args.state, sizeof (st), cxt->hip->stream) || arthip_sync (cxt->hip->stream)) return;
    cxt->tail = st [0].mark; cxt->head = st [0].fill; cxt->outsamples_error = st [0].drift;
    if (cxt->next) { cxt->next->tail = st [1].mark; cxt->next->head = st [1].fill; cxt->next->outsamples_error = st [1].drift; }
}

static Stretch *make_stage (int shortest, int longest, int channels, int fast)
{
    Stretch *s = calloc (1, sizeof (*s));
    if (!s) return NULL;
    s->num_chans = channels;
    s->inbuff_samples = longest * channels * (fast ? 4 : 3);
    s->head = s->tail = s->longest = longest * channels;
    s->shortest = shortest * channels;
    s->fast_mode = fast;
    return s;
}

Stretch *stretchInit (int shortest_period, int longest_period, int num_channels, int flags)
{
    const int fast = (flags & STRETCH_FAST_FLAG) != 0, dual = (flags & STRETCH_DUAL_FLAG) != 0;

    if (fast) {
        longest_period = (longest_period + 1) & ~1;
        shortest_period &= ~1;
    }

    if (longest_period <= shortest_period || shortest_period < MIN_PERIOD || longest_period > MAX_PERIOD) {
        fprintf (stderr, "stretchInit(): invalid periods!\n");
        return NULL;
    }

    if (num_channels < 1 || num_channels > 2) {
        fprintf (stderr, "stretchInit(): mono or stereo only!\n");
        return NULL;
    }

    if (artamdDeviceCount () <= 0) {
        fprintf (stderr, "artamd: stretchInit needs a HIP device (no CPU path): %s\n", arthip_last_error ());
        return NULL;
    }

    Stretch *cxt = make_stage (shortest_period, longest_period, num_channels, fast);
    struct artamd_stretch *hip = calloc (1, sizeof (*hip));
    if (!cxt || !hip) { free (cxt); free (hip); fprintf (stderr, "stretchInit(): out of memory!\n"); return NULL; }
    cxt->hip = hip;
    if (dual && !(cxt->next = make_stage (shortest_period, longest_period, num_channels, fast))) { stretchFree (cxt); return NULL; }

    ArtStretchArgs *a = &hip->args;
    const size_t ring_bytes = sizeof (art_s) * (size_t) cxt->inbuff_samples;
    int failed = 0;
    hip->blocks = fast ? 4 : 3;
    a->channels = num_channels; a->room = cxt->inbuff_samples; a->lo = cxt->shortest; a->hi = cxt->longest;
    a->quick = fast; a->paired = dual;
    for (int s = 0; s < (dual ? 2 : 1); ++s)
        for (int b = 0; b < 2; ++b) {
            a->ring [s][b] = arthip_malloc (ring_bytes);
            failed |= !a->ring [s][b] || arthip_zero (a->ring [s][b], ring_bytes, NULL);
        }
    if (dual) { a->between = arthip_malloc (ring_bytes); failed |= !a->between; }
    a->total = arthip_malloc (sizeof (art_s) * (MAX_PERIOD + 8));
    a->score = arthip_malloc (sizeof (art_s) * (MAX_PERIOD + 8));
    a->state = arthip_malloc (2 * sizeof (DevState));
    hip->d_result = arthip_malloc (sizeof (int));
    failed |= !a->total || !a->score || !a->state || !hip->d_result;

    if (failed || push_state (cxt)) {
        fprintf (stderr, "artamd: stretchInit: device allocation failed: %s\n", arthip_last_error ());
        stretchFree (cxt);
        return NULL;
    }

    return cxt;
}

void stretchFree (Stretch *cxt)
{
    if (!cxt) return;
    if (cxt->hip) {
        ArtStretchArgs *a = &cxt->hip->args;
        for (int s = 0; s < 2; ++s) for (int b = 0; b < 2; ++b) arthip_free (a->ring [s][b]);
        arthip_free (a->between); arthip_free (a->total); arthip_free (a->score); arthip_free (a->state);
        arthip_free (cxt->hip->d_result); arthip_free (cxt->hip->d_in); arthip_free (cxt->hip->d_out); arthip_free (cxt->hip->d_batch);
        free (cxt->hip);
    }
    free (cxt->next);
    free (cxt);
}

void stretchReset (Stretch *cxt)
{
    ArtStretchArgs *a = &cxt->hip->args;
    /* the reference keeps outsamples_error across a reset (stretch.c:102-110) — so do we */
    for (Stretch *s = cxt; s; s = s->next) s->head = s->tail = s->longest;
    for (int s = 0; s < (a->paired ? 2 : 1); ++s)
        arthip_zero (a->ring [s][0], sizeof (art_s) * (size_t) cxt->longest, cxt->hip->stream);
    push_state (cxt);                                   /* ring 0 current again */
}

int stretchGetOutputCapacity (Stretch *cxt, int max_num_samples, double max_ratio)
{
    int frames = max_num_samples;

    for (Stretch *s = cxt; s; s = s->next) {            /* stage by stage, as the reference recurses (stretch.c:117-143) */
        double here = max_ratio, rest = 1.0;
        if (s->next) {
            if (here < 0.5) { rest = here / 0.5; here = 0.5; }
            else if (here > 2.0) { rest = here / 2.0; here = 2.0; }
        }
        frames = (int) ceil (frames * ceil (here * 2.0) / 2.0) + (s->longest / s->num_chans) * (s->fast_mode ? 4 : 3);
        max_ratio = rest;
    }

    return frames;
}

/* (rings and state are shared between calls: the old stream is drained before the switch) */
void stretchHipSetStream (Stretch *cxt, void *hipStream)
{
    if (cxt->hip->stream == hipStream) return;
    arthip_sync (cxt->hip->stream);
    cxt->hip->stream = hipStream;
}

static int device_call (Stretch *cxt, const art_s *d_in, int frames, art_s *d_out, double ratio, int flush)
{
    struct artamd_stretch *hip = cxt->hip;
    int made = 0;

    if (arthip_stretch_call (&hip->args, d_in, frames, d_out, ratio, flush, hip->d_result, hip->stream) ||
        arthip_d2h (&made, hip->d_result, sizeof (int), hip->stream) || arthip_sync (hip->stream)) {
        fprintf (stderr, "artamd: stretch launch failed: %s\n", arthip_last_error ());
        return 0;
    }

    pull_state (cxt);
    return made;
}

int stretchProcessDevice (Stretch *cxt, const artsample_t *d_samples, int num_samples, artsample_t *d_output, double ratio)
{
    return num_samples > 0 ? device_call (cxt, d_samples, num_samples, d_output, ratio, 0) : 0;
}

int stretchFlushDevice (Stretch *cxt, artsample_t *d_output)
{
    return device_call (cxt, NULL, 0, d_output, 1.0, 1);
}

/* n independent streams, one launch: item i is exactly the call stretchProcessDevice (cxts [i], ...) / stretchFlushDevice
 * would make — same device code, one workgroup per stream — so results are identical to n separate calls.  The launch
 * goes to the stream of cxts [0], whose scratch also carries the item table. */
static unsigned long *stamp_of (const void *cxt) { return &((const Stretch *) cxt)->hip->batch_stamp; }

/* what a batched launch reports for one context: the frame count, and the host mirrors of the state it left */
static void mirror_state (Stretch *c, const ArtStretchDone *done, int *produced)
{
    *produced = done->made;
    c->tail = done->state [0].mark; c->head = done->state [0].fill; c->outsamples_error = done->state [0].drift;
    if (c->next) { c->next->tail = done->state [1].mark; c->next->head = done->state [1].fill; c->next->outsamples_error = done->state [1].drift; }
}

static int batch_call (Stretch *const *cxts, int n, const artsample_t *const *d_samples, const int *num_samples,
                       artsample_t *const *d_outputs, const double *ratios, int flush, int *produced)
{
    if (n <= 0) return 0;
    struct artamd_stretch *lead = cxts [0]->hip;
    const size_t items_bytes = ((size_t) n * sizeof (ArtStretchItem) + 63) & ~(size_t) 63, done_bytes = (size_t) n * sizeof (ArtStretchDone);
    ArtStretchItem *items = malloc (items_bytes);
    ArtStretchDone *done = malloc (done_bytes);
    int rc = -1;

    lead->d_batch = arthip_grow (lead->d_batch, &lead->batch_cap, items_bytes + done_bytes);
    if (!items || !done || !lead->d_batch || artamd_batch_distinct ((const void *const *) cxts, n, stamp_of, "stretch", "context")) goto out;

    for (int i = 0; i < n; ++i) {
        items [i].args = cxts [i]->hip->args;
        items [i].in = flush ? NULL : d_samples [i];
        items [i].out = d_outputs [i];
        items [i].ratio = flush ? 1.0 : ratios [i];
        items [i].frames = flush ? 0 : num_samples [i];
        /* a stream with nothing to process this round still takes part: its workgroup returns at once */
        items [i].flush = flush;
    }

    ArtStretchDone *d_done = (ArtStretchDone *)((char *) lead->d_batch + items_bytes);
    if (arthip_h2d (lead->d_batch, items, (size_t) n * sizeof (ArtStretchItem), lead->stream) ||
        arthip_stretch_batch ((const ArtStretchItem *) lead->d_batch, d_done, n, lead->stream) ||
        arthip_d2h (done, d_done, done_bytes, lead->stream) || arthip_sync (lead->stream)) {
        fprintf (stderr, "artamd: stretch batch launch failed: %s\n", arthip_last_error ());
        goto out;
    }

    for (int i = 0; i < n; ++i) mirror_state (cxts [i], &done [i], &produced [i]);
    rc = 0;
out:
    free (items); free (done);
    return rc;
}

int stretchProcessBatchDevice (Stretch *const *cxts, int n, const artsample_t *const *d_samples, const int *num_samples,
                               artsample_t *const *d_outputs, const double *ratios, int *produced)
{
    return batch_call (cxts, n, d_samples, num_samples, d_outputs, ratios, 0, produced);
}

int stretchFlushBatchDevice (Stretch *const *cxts, int n, artsample_t *const *d_outputs, int *produced)
{
    return batch_call (cxts, n, NULL, NULL, d_outputs, NULL, 1, produced);
}

/* Frames a whole clip can emit, process call and every flush together, from ANY state of the context: a stage holds at most its
 * ring of values beside what comes in, each of them is consumed by one step or flushed once, a flush emits at 1, and a step emits
 * at most ceil (2 r) / 2 values per value it consumes (r: the stage's clipped ratio; 0.5: p for 2p, 1: 2p for 2p, 1.5: 3p for 2p,
 * 2: 2p for p, and the drift only chooses between floor and ceil of 2 r).  A ratio that is not a number takes the 2:1 step. */
static long long stage_bound (long long frames, int longest, int fast, double ratio)
{
    const double r = ratio < 0.5 ? 0.5 : ratio;
    const double gain = !(r <= 2.0) ? 2.0 : fmax (1.0, ceil (r * 2.0) / 2.0);
    return (long long) ceil ((double)(frames + (long long) longest * (fast ? 4 : 3)) * gain);
}

int artamdStretchClipCapacity (int longest_period, int flags, int num_samples, double ratio)
{
    const int fast = (flags & STRETCH_FAST_FLAG) != 0, dual = (flags & STRETCH_DUAL_FLAG) != 0;
    double here = ratio, rest = 1.0;

    if (fast) longest_period = (longest_period + 1) & ~1;
    if (longest_period < 1 || longest_period > MAX_PERIOD) return -1;
    if (num_samples < 0) num_samples = 0;
    if (dual) {                                         /* as stretchGetOutputCapacity splits the ratio */
        if (here < 0.5) { rest = here / 0.5; here = 0.5; }
        else if (here > 2.0) { rest = here / 2.0; here = 2.0; }
    }
    long long frames = stage_bound (num_samples, longest_period, fast, here);
    if (dual) frames = stage_bound (frames, longest_period, fast, rest);
    return frames > 0x7fffffff ? -1 : (int) frames;     /* (-1: more than an int holds) */
}

/* Segments a stage can write (art_hip.h).  A step needs the mark to move on by its period at least (p for the 2:1 step, 2 p for the
 * others; the quick 2:1 step makes two fades and moves on by 2 p) and p is never below the shortest period, so a stage that is fed
 * `fed` frames in all takes at most fed / shortest steps, of three segments at the most (the 3:2 step).  Beyond the steps a stage
 * writes one segment per feed call that ends in the pass-through, and one per flush (drain's pending copy), of which the clip kernel
 * makes four at the most.  Stage 0 is fed once.  Stage 1 is fed once per step of stage 0, once by stage 0's pass-through and once per
 * flush of stage 0, and what it is fed in all is what stage 0 makes: at most stage_bound (). */
int artamdStretchLogCapacity (int shortest_period, int longest_period, int flags, int num_samples, double ratio, int stage)
{
    const int fast = (flags & STRETCH_FAST_FLAG) != 0, dual = (flags & STRETCH_DUAL_FLAG) != 0;
    double here = ratio;

    if (artamdStretchClipCapacity (longest_period, flags, num_samples, ratio) < 0) return -1;
    if (fast) { longest_period = (longest_period + 1) & ~1; shortest_period &= ~1; }
    if (shortest_period < 1 || stage < 0 || stage > 1) return -1;
    if (stage == 1 && !dual) return 0;
    if (num_samples < 0) num_samples = 0;
    const long long steps0 = num_samples / shortest_period;
    long long segments = 3 * steps0 + 1 + 4;
    if (stage == 1) {
        if (here < 0.5) here = 0.5; else if (here > 2.0) here = 2.0;     /* stage 0's share of the ratio */
        const long long fed = stage_bound (num_samples, longest_period, fast, here);
        segments = 3 * (fed / shortest_period) + (steps0 + 1 + 4) + 4;
    }
    return segments > 0x7fffffff ? -1 : (int) segments;
}

/* Whole clips in ONE launch and one synchronisation: art_hip.h.  Everything is checked before anything is enqueued.  With d_logs the
 * logging kernel, from a fresh start, and the segment counts in the same read-back. */
static int clips_call (Stretch *const *cxts, int n, const artsample_t *const *d_samples, const long *inputPitches,
                       const int *num_samples, artsample_t *const *d_outputs, const long *outputPitches,
                       const int *outputCaps, const double *ratios, int fromStart, int *produced,
                       ArtamdStretchSegment *const *d_logs, const int *logCaps, int *logCounts, int logged)
{
    if (n <= 0) return 0;
    if (!cxts || !num_samples || !d_outputs || !outputCaps || !ratios || !produced) return -1;
    if (logged && (!d_logs || !logCaps || !logCounts)) return -1;
    for (int i = 0; i < n; ++i) {
        const Stretch *c = cxts [i];
        if (!c || !c->hip) return -1;
        for (int s = 0; logged && s < (c->next ? 2 : 1); ++s) {
            const int segments = artamdStretchLogCapacity (c->shortest / c->num_chans, c->longest / c->num_chans,
                                                           (c->fast_mode ? STRETCH_FAST_FLAG : 0) | (c->next ? STRETCH_DUAL_FLAG : 0), num_samples [i], ratios [i], s);
            if (!d_logs [2 * i + s] || segments < 0 || logCaps [2 * i + s] < segments) return -1;
        }
        const int need = artamdStretchClipCapacity (c->longest / c->num_chans, (c->fast_mode ? STRETCH_FAST_FLAG : 0) | (c->next ? STRETCH_DUAL_FLAG : 0),
                                                    num_samples [i], ratios [i]);
        if (!d_outputs [i] || (num_samples [i] > 0 && (!d_samples || !d_samples [i])) || need < 0 || outputCaps [i] < need) return -1;
        /* planes must not run into one another: a pitch holds the clip, the output's everything the clip can emit */
        const long in_pitch = inputPitches ? inputPitches [i] : 0, out_pitch = outputPitches ? outputPitches [i] : 0;
        if (c->num_chans > 1 && ((in_pitch && in_pitch < num_samples [i]) || (out_pitch && out_pitch < need))) return -1;
    }
    if (artamd_batch_distinct ((const void *const *) cxts, n, stamp_of, "stretch", "context")) return -1;

    struct artamd_stretch *lead = cxts [0]->hip;
    /* the table: the clips, then (logged) their log pointers; what comes back: the results, then (logged) two counts per clip */
    const size_t clips_bytes = ((size_t) n * sizeof (ArtStretchClip) + 63) & ~(size_t) 63;
    const size_t items_bytes = clips_bytes + (logged ? ((size_t) n * sizeof (ArtStretchLogs) + 63) & ~(size_t) 63 : 0);
    const size_t results_bytes = (size_t) n * sizeof (ArtStretchDone), done_bytes = results_bytes + (logged ? (size_t) n * 2 * sizeof (int) : 0);
    ArtStretchClip *items = malloc (items_bytes);
    ArtStretchDone *done = malloc (done_bytes);
    int rc = -1;

    lead->d_batch = arthip_grow (lead->d_batch, &lead->batch_cap, items_bytes + done_bytes);
    if (!items || !done || !lead->d_batch) goto out;
    ArtStretchLogs *logs = (ArtStretchLogs *)((char *) items + clips_bytes);

    for (int i = 0; i < n; ++i) {
        items [i].args = cxts [i]->hip->args;
        items [i].in = num_samples [i] > 0 ? d_samples [i] : NULL;
        items [i].out = d_outputs [i];
        items [i].in_pitch = inputPitches ? inputPitches [i] : 0;
        items [i].out_pitch = outputPitches ? outputPitches [i] : 0;
        items [i].ratio = ratios [i];
        items [i].frames = num_samples [i] > 0 ? num_samples [i] : 0;
        items [i].from_start = fromStart != 0;
        if (logged) { logs [i].seg [0] = d_logs [2 * i]; logs [i].seg [1] = cxts [i]->next ? d_logs [2 * i + 1] : NULL; }
    }

    ArtStretchDone *d_done = (ArtStretchDone *)((char *) lead->d_batch + items_bytes);
    if (arthip_h2d (lead->d_batch, items, logged ? clips_bytes + (size_t) n * sizeof (ArtStretchLogs) : (size_t) n * sizeof (ArtStretchClip), lead->stream) ||
        (logged ? arthip_stretch_clips_logged ((const ArtStretchClip *) lead->d_batch, d_done, (const ArtStretchLogs *)((char *) lead->d_batch + clips_bytes),
                                               (int *)((char *) d_done + results_bytes), n, lead->stream)
                : arthip_stretch_clips ((const ArtStretchClip *) lead->d_batch, d_done, n, lead->stream)) ||
        arthip_d2h (done, d_done, done_bytes, lead->stream) || arthip_sync (lead->stream)) {
        fprintf (stderr, "artamd: stretch clip launch failed: %s\n", arthip_last_error ());
        artamd_note_failure ("stretch: the whole-clip launch failed");
        goto out;
    }

    for (int i = 0; i < n; ++i) mirror_state (cxts [i], &done [i], &produced [i]);
    if (logged) memcpy (logCounts, (const char *) done + results_bytes, (size_t) n * 2 * sizeof (int));
    rc = 0;
out:
    free (items); free (done);
    return rc;
}

int stretchProcessAndFlushBatchPlanarDevice (Stretch *const *cxts, int n, const artsample_t *const *d_samples, const long *inputPitches,
                                             const int *num_samples, artsample_t *const *d_outputs, const long *outputPitches,
                                             const int *outputCaps, const double *ratios, int fromStart, int *produced)
{
    return clips_call (cxts, n, d_samples, inputPitches, num_samples, d_outputs, outputPitches, outputCaps, ratios, fromStart, produced, NULL, NULL, NULL, 0);
}

int stretchProcessAndFlushLoggedBatchPlanarDevice (Stretch *const *cxts, int n, const artsample_t *const *d_samples, const long *inputPitches,
                                                   const int *num_samples, artsample_t *const *d_outputs, const long *outputPitches,
                                                   const int *outputCaps, const double *ratios, int *produced,
                                                   ArtamdStretchSegment *const *d_logs, const int *logCaps, int *logCounts)
{
    return clips_call (cxts, n, d_samples, inputPitches, num_samples, d_outputs, outputPitches, outputCaps, ratios, 1, produced, d_logs, logCaps, logCounts, 1);
}

/* The gradient of logged clips: art_hip.h.  Everything is checked before anything is enqueued; the contexts are only read.  The table
 * (one item per stage) and the pairs' intermediate gradients ride in the lead context's batch buffer. */
int stretchAdjointClipsPlanarDevice (Stretch *const *cxts, int n, const ArtamdStretchSegment *const *d_logs, const int *logCounts,
                                     const artsample_t *const *d_gouts, const long *goutPitches, const int *n_outs,
                                     artsample_t *const *d_gins, const long *ginPitches, const int *n_ins)
{
    if (n <= 0) return 0;
    if (!cxts || !d_logs || !logCounts || !d_gouts || !n_outs || !d_gins || !n_ins) return -1;
    int last = 0, first = 0;                            /* items of the two launches */
    size_t mid_values = 0;
    for (int i = 0; i < n; ++i) {
        const Stretch *c = cxts [i];
        if (!c || !c->hip || n_ins [i] < 0 || n_outs [i] < 0) return -1;
        for (int s = 0; s < (c->next ? 2 : 1); ++s)
            if (logCounts [2 * i + s] < 0 || (logCounts [2 * i + s] > 0 && !d_logs [2 * i + s])) return -1;
        if (!n_ins [i]) continue;                       /* (nothing to write: the item takes no further part) */
        for (int s = 0; s < (c->next ? 2 : 1); ++s) {   /* (a count above what n_ins [i] frames can log at any ratio is not this clip's) */
            const int cap = artamdStretchLogCapacity (c->shortest / c->num_chans, c->longest / c->num_chans,
                                                      (c->fast_mode ? STRETCH_FAST_FLAG : 0) | (c->next ? STRETCH_DUAL_FLAG : 0), n_ins [i], 2.0, s);
            if (logCounts [2 * i + s] > cap) return -1;
        }
        const long gy_pitch = goutPitches ? goutPitches [i] : 0, gx_pitch = ginPitches ? ginPitches [i] : 0;
        if (!d_gins [i] || (n_outs [i] > 0 && !d_gouts [i])) return -1;
        if (c->num_chans > 1 && ((gy_pitch && gy_pitch < n_outs [i]) || (gx_pitch && gx_pitch < n_ins [i]))) return -1;
        const long long values = (long long) n_ins [i] * c->num_chans, outs = (long long) n_outs [i] * c->num_chans;
        const long long mid = c->next ? stage_bound (n_ins [i], c->longest / c->num_chans, c->fast_mode, 2.0) * c->num_chans : 0;
        if (values > 0x7fffffff || outs > 0x7fffffff || mid > 0x7fffffff) return -1;
        ++last;
        if (c->next) { ++first; mid_values += (size_t) mid; }
    }
    if (!last) return 0;

    struct artamd_stretch *lead = cxts [0]->hip;
    const size_t table_bytes = ((size_t)(last + first) * sizeof (ArtStretchAdjItem) + 63) & ~(size_t) 63;
    ArtStretchAdjItem *items = calloc ((size_t)(last + first), sizeof (ArtStretchAdjItem));
    int rc = -1, launches = 0;

    lead->d_batch = arthip_grow (lead->d_batch, &lead->batch_cap, table_bytes + mid_values * sizeof (art_s));
    if (!items || !lead->d_batch) goto out;

    art_s *d_mid = (art_s *)((char *) lead->d_batch + table_bytes);
    ArtStretchAdjItem *a = items, *b = items + last;   /* the stage that wrote the output; the pairs' first stage */
    for (int i = 0; i < n; ++i) {
        const Stretch *c = cxts [i];
        if (!n_ins [i]) continue;
        const int C = c->num_chans;
        a->channels = C; a->back = c->longest; a->ahead = c->inbuff_samples;
        a->gy = d_gouts [i]; a->gy_pitch = C > 1 && goutPitches ? goutPitches [i] : 0; a->gy_values = n_outs [i] * C;
        if (!c->next) {
            a->log = d_logs [2 * i]; a->count = logCounts [2 * i];
            a->gx = d_gins [i]; a->gx_pitch = C > 1 && ginPitches ? ginPitches [i] : 0; a->gx_values = n_ins [i] * C;
        }
        else {
            const int mid = (int)(stage_bound (n_ins [i], c->longest / C, c->fast_mode, 2.0) * C);
            a->log = d_logs [2 * i + 1]; a->count = logCounts [2 * i + 1];
            a->mid = d_logs [2 * i]; a->mid_count = logCounts [2 * i]; a->mid_is_gx = 1;
            a->gx = d_mid; a->gx_pitch = 0; a->gx_values = mid;
            *b = *a;
            b->log = d_logs [2 * i]; b->count = logCounts [2 * i]; b->mid_is_gx = 0;
            b->gy = d_mid; b->gy_pitch = 0; b->gy_values = mid;
            b->gx = d_gins [i]; b->gx_pitch = C > 1 && ginPitches ? ginPitches [i] : 0; b->gx_values = n_ins [i] * C;
            ++b;
            d_mid += mid;
        }
        ++a;
    }

    if (arthip_stretch_adjoint (items, last, lead->d_batch, lead->stream) ||
        (++launches, first && arthip_stretch_adjoint (items + last, first, (ArtStretchAdjItem *) lead->d_batch + last, lead->stream))) {
        fprintf (stderr, "artamd: stretch adjoint launch failed: %s\n", arthip_last_error ());
        artamd_note_failure ("stretch: the adjoint launch failed");
        goto out;
    }
    rc = launches + (first ? 1 : 0);
out:
    free (items);
    return rc;
}

/* frames a call can emit at most: what is buffered plus what comes in, at the largest stage ratios, plus slack */
static size_t worst_case_frames (Stretch *cxt, int num_samples)
{
    size_t frames = (size_t) num_samples + (size_t) cxt->inbuff_samples / cxt->num_chans;
    for (Stretch *s = cxt; s; s = s->next)
        frames = frames * 2 + (size_t)(s->inbuff_samples / s->num_chans) * 2;
    return frames;
}

int stretchProcess (Stretch *cxt, const artsample_t *samples, int num_samples, artsample_t *output, double ratio)
{
    struct artamd_stretch *hip = cxt->hip;
    const int C = cxt->num_chans;

    if (num_samples <= 0) return 0;
    hip->d_in = arthip_grow (hip->d_in, &hip->in_cap, sizeof (art_s) * (size_t) num_samples * C);
    hip->d_out = arthip_grow (hip->d_out, &hip->out_cap, sizeof (art_s) * worst_case_frames (cxt, num_samples) * C);
    if (!hip->d_in || !hip->d_out || arthip_h2d (hip->d_in, samples, sizeof (art_s) * (size_t) num_samples * C, hip->stream)) {
        fprintf (stderr, "artamd: stretchProcess: %s\n", arthip_last_error ());
        return 0;
    }

    const int made = device_call (cxt, hip->d_in, num_samples, hip->d_out, ratio, 0);
    if (made > 0) { arthip_d2h (output, hip->d_out, sizeof (art_s) * (size_t) made * C, hip->stream); arthip_sync (hip->stream); }
    return made;
}

int stretchFlush (Stretch *cxt, artsample_t *output)
{
    struct artamd_stretch *hip = cxt->hip;
    const int C = cxt->num_chans;

    hip->d_out = arthip_grow (hip->d_out, &hip->out_cap, sizeof (art_s) * worst_case_frames (cxt, 0) * C);
    if (!hip->d_out) return 0;
    const int made = device_call (cxt, NULL, 0, hip->d_out, 1.0, 1);
    if (made > 0) { arthip_d2h (output, hip->d_out, sizeof (art_s) * (size_t) made * C, hip->stream); arthip_sync (hip->stream); }
    return made;
}
