/* pcm_host.c — host (C) side of the biquad and decimator entry points.
 *
 * Host work: coefficient design (reference biquad.c:18-74, decimator.c:28-97, :389-409) and moving
 * caller buffers to/from HBM.  Every sample is processed by the kernels in pcm_kernels.hip.
 */
#define _USE_MATH_DEFINES
#include <limits.h>
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "art_internal.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

/* ------------------------------------------------------------------------------------------
 * Biquad design
 * ---------------------------------------------------------------------------------------- */

/* The void entry points of the reference (biquad_apply_*, floatIntegersLE) cannot report a failure, and there is no CPU path to
 * fall back to: a failure is printed, counted (artamdErrorCount / artamdLastError: tools check them before they trust the audio
 * they write) and, with ARTAMD_ABORT_ON_ERROR=1, fatal on the spot. */
static int pcm_errors;
static char pcm_last_error [256], pcm_last_error_out [256];
static pthread_mutex_t pcm_error_lock = PTHREAD_MUTEX_INITIALIZER;      /* (callers hold different locks: the message has its own) */
static void pcm_fail (const char *what)
{
    static int abort_on_error = -1;
    pthread_mutex_lock (&pcm_error_lock);
    if (abort_on_error < 0) { const char *e = getenv ("ARTAMD_ABORT_ON_ERROR"); abort_on_error = e && *e && *e != '0'; }
    snprintf (pcm_last_error, sizeof (pcm_last_error), "%s: %s", what, arthip_last_error ());
    fprintf (stderr, "artamd: %s\n", pcm_last_error);
    __atomic_add_fetch (&pcm_errors, 1, __ATOMIC_RELAXED);
    const int fatal = abort_on_error;
    pthread_mutex_unlock (&pcm_error_lock);
    if (fatal) abort ();
}
/* (the resampler's entry points report a failed launch the same way: resampler_host.c) */
void artamd_note_failure (const char *what) { pcm_fail (what); }
int artamdErrorCount (void) { return __atomic_load_n (&pcm_errors, __ATOMIC_RELAXED); }
const char *artamdLastError (void)
{
    if (!artamdErrorCount ()) return NULL;
    pthread_mutex_lock (&pcm_error_lock);               /* (a whole message, never a torn one) */
    memcpy (pcm_last_error_out, pcm_last_error, sizeof (pcm_last_error_out));
    pthread_mutex_unlock (&pcm_error_lock);
    return pcm_last_error_out;
}

static void butterworth (double freq, double *K_out, double *norm_out, double *b1, double *b2)
{
    const double Q = sqrt (0.5), K = tan (M_PI * freq);
    const double norm = 1.0 / (1.0 + K / Q + K * K);
    *K_out = K; *norm_out = norm;
    *b1 = 2.0 * (K * K - 1.0) * norm;
    *b2 = (1.0 - K / Q + K * K) * norm;
}

void biquad_lowpass (BiquadCoefficients *filter, double frequency)
{
    double K, norm, b1, b2;
    butterworth (frequency, &K, &norm, &b1, &b2);
    memset (filter, 0, sizeof (*filter));
    filter->a0 = (art_s)(K * K * norm);
    filter->a1 = (art_s)(2 * filter->a0);       /* doubled AFTER rounding to art_s (reference biquad.c:26) */
    filter->a2 = filter->a0;
    filter->b1 = (art_s) b1;
    filter->b2 = (art_s) b2;
}

void biquad_highpass (BiquadCoefficients *filter, double frequency)
{
    double K, norm, b1, b2;
    butterworth (frequency, &K, &norm, &b1, &b2);
    memset (filter, 0, sizeof (*filter));
    filter->a0 = (art_s) norm;
    filter->a1 = (art_s)(-2.0 * norm);
    filter->a2 = filter->a0;
    filter->b1 = (art_s) b1;
    filter->b2 = (art_s) b2;
}

void biquad_init (Biquad *f, const BiquadCoefficients *c, double gain)
{
    memset (f, 0, sizeof (*f));
    f->a [0] = (art_s)(c->a0 * gain); f->a [1] = (art_s)(c->a1 * gain); f->a [2] = (art_s)(c->a2 * gain);
    f->a [3] = (art_s)(c->a3 * gain); f->a [4] = (art_s)(c->a4 * gain);
    f->b [1] = c->b1; f->b [2] = c->b2; f->b [3] = c->b3; f->b [4] = c->b4;
    f->order = (c->a4 != 0.0F || c->b4 != 0.0F) ? 4 : (c->a3 != 0.0F || c->b3 != 0.0F) ? 3 :
               (c->a2 != 0.0F || c->b2 != 0.0F) ? 2 : 1;
}

/* ------------------------------------------------------------------------------------------
 * How the cascades run.  A biquad is a serial recurrence through float rounding; the bit-exact form that is parallel over
 * TIME (pcm_kernels.hip, biquad_spec_kernel) needs to know how fast the recursive part forgets its state: the warm-up W
 * is the number of frames after which every unit initial state has decayed below 2^-40 (2^-70 for 8-byte samples; + margin).  Filters that do not
 * forget within SPEC_MAX_WARMUP frames (poles within ~0.97 of the unit circle) and short runs take the serial kernels.
 * Both forms produce the reference's bits (biquad.c:106-163); ARTAMD_BIQUAD_SERIAL=1 forces the serial one.
 * ---------------------------------------------------------------------------------------- */
#define SPEC_MAX_WARMUP 1024

static int forget_length (const Biquad *f)
{
    const int order = f->order;
    int worst = 0;

    if (order < 1 || order > 4) return 0;
    for (int j = 0; j < order; ++j) {
        double y [4] = { 0.0, 0.0, 0.0, 0.0 };
        int last = 0;
        y [j] = 1.0;
        for (int n = 1; n <= SPEC_MAX_WARMUP + 64; ++n) {
            double v = 0.0;
            for (int k = 1; k <= order; ++k) v -= (double) f->b [k] * y [k - 1];
            y [3] = y [2]; y [2] = y [1]; y [1] = y [0]; y [0] = v;
            if (!(fabs (v) <= (ART_WIDE ? 0x1p-70 : 0x1p-40))) last = n;        /* (also catches a blow-up: inf / NaN) */
        }
        if (last > worst) worst = last;
    }
    /* ARTAMD_BIQUAD_WARMUP=n forces the warm-up (tests: a warm-up far too short makes nearly every chunk boundary mismatch,
     * which exercises the verification and repair path; the results must not change) */
    { const char *e = getenv ("ARTAMD_BIQUAD_WARMUP"); if (e && *e) return atoi (e); }
    return worst > SPEC_MAX_WARMUP ? 0 : worst + 16;
}

/* The route rule: the chunk length if a call of `frames` frames through `sections` sections with warm-up W each (0: none forgets)
 * takes the time-parallel form, else 0.  The warm-up is recomputed work: the chunk keeps it to about a quarter, and a call has two. */
static int spec_chunk (int sections, int W, int frames)
{
    if (!W) return 0;
    int L = 4 * sections * W;
    L = (L + 7) & ~7;
    if (L < 128) L = 128;
    if (L > 8192) L = 8192;
    return frames >= 2 * L ? L : 0;
}

/* ... and the rule of the entries that gather calls: a call goes the time-parallel way there if its single call would AND it is
 * longer than serialMax frames (BQ_BATCH_SERIAL_MAX below: up to there one serial lane of a shared launch is faster) */
static int gathered_chunk (int sections, int W, int frames, int serialMax) { return frames > serialMax ? spec_chunk (sections, W, frames) : 0; }

static int spec_disabled (void)
{
    static int cached = -1;
    if (cached < 0) { const char *e = getenv ("ARTAMD_BIQUAD_SERIAL"); cached = e && *e && *e != '0'; }
    return cached;
}

/* ------------------------------------------------------------------------------------------
 * Biquad, host-pointer entry points (what ART's -p filters call, art.c:1011-1017, :1052-1058: one section of one channel
 * of an interleaved buffer per call).  Only the channel's own samples travel: gathered by the CPU into page-locked
 * staging, one DMA each way, the time-parallel kernel on a dense run, scattered back.  Process-wide scratch.
 * ---------------------------------------------------------------------------------------- */

static pthread_mutex_t scratch_lock = PTHREAD_MUTEX_INITIALIZER;
static struct {
    art_s *d_in, *d_out; size_t cap;                   /* samples */
    art_s *h_buf; size_t h_cap;                        /* page-locked, samples */
    Biquad *d_state, *h_state;
    void *d_spec; size_t spec_cap;
    unsigned int *d_repairs;
    int *d_first_bad;
    int device;
} host_scratch = { .device = -1 };

static int scratch_reserve (size_t samples)
{
    const int device = arthip_current_device ();
    if (host_scratch.device != device) {                /* first use (or the caller moved to another GPU): start over there */
        arthip_free (host_scratch.d_in); arthip_free (host_scratch.d_out); arthip_free (host_scratch.d_state);
        arthip_free (host_scratch.d_spec); arthip_free (host_scratch.d_repairs); arthip_free (host_scratch.d_first_bad);
        arthip_host_free (host_scratch.h_buf); arthip_host_free (host_scratch.h_state);
        memset (&host_scratch, 0, sizeof (host_scratch));
        host_scratch.device = device;
    }
    if (!host_scratch.d_state && !(host_scratch.d_state = arthip_malloc (sizeof (Biquad)))) return -1;
    if (!host_scratch.h_state && !(host_scratch.h_state = arthip_host_alloc (sizeof (Biquad)))) return -1;
    if (!host_scratch.d_repairs) {
        if (!(host_scratch.d_repairs = arthip_malloc (sizeof (unsigned int)))) return -1;
        arthip_zero (host_scratch.d_repairs, sizeof (unsigned int), NULL);
    }
    if (!host_scratch.d_first_bad) {
        if (!(host_scratch.d_first_bad = arthip_malloc (sizeof (int)))) return -1;
        arthip_biquad_spec_arm (host_scratch.d_first_bad, 1, NULL);
    }
    if (samples > host_scratch.cap) {
        arthip_free (host_scratch.d_in); arthip_free (host_scratch.d_out);
        host_scratch.cap = samples + samples / 2 + 1024;
        host_scratch.d_in = arthip_malloc (host_scratch.cap * sizeof (art_s));
        host_scratch.d_out = arthip_malloc (host_scratch.cap * sizeof (art_s));
        if (!host_scratch.d_in || !host_scratch.d_out) { host_scratch.cap = 0; return -1; }
    }
    if (samples > host_scratch.h_cap) {
        arthip_host_free (host_scratch.h_buf);
        host_scratch.h_cap = samples + samples / 2 + 1024;
        if (!(host_scratch.h_buf = arthip_host_alloc (host_scratch.h_cap * sizeof (art_s)))) { host_scratch.h_cap = 0; return -1; }
    }
    return 0;
}

static void biquad_run_host (Biquad *f, art_s *buffer, int n, int stride, int sample_form)
{
    if (n <= 0) return;

    pthread_mutex_lock (&scratch_lock);
    if (arthip_device_count () < 1 || scratch_reserve ((size_t) n)) {
        /* no CPU evaluation path exists: say so (counted: artamdErrorCount) and leave the caller's samples and filter state untouched */
        pcm_fail ("biquad needs a HIP device and scratch memory (no CPU path)");
        pthread_mutex_unlock (&scratch_lock);
        return;
    }

    art_s *h = host_scratch.h_buf;
    if (stride == 1) memcpy (h, buffer, sizeof (art_s) * (size_t) n);
    else for (int i = 0; i < n; ++i) h [i] = buffer [(size_t) i * stride];
    *host_scratch.h_state = *f;
    /* samples and filter state travel in one launch each way (a copy kernel over the page-locked buffers; beyond a megabyte
     * the copy engines) */
    const int by_kernel = sizeof (art_s) * (size_t) n <= ((size_t) 1 << 20);
    if (by_kernel)
        arthip_copy2_by_kernel (host_scratch.d_in, h, sizeof (art_s) * (size_t) n, host_scratch.d_state, host_scratch.h_state, sizeof (Biquad), NULL);
    else {
        arthip_h2d (host_scratch.d_in, h, sizeof (art_s) * (size_t) n, NULL);
        arthip_h2d (host_scratch.d_state, host_scratch.h_state, sizeof (Biquad), NULL);
    }

    const int W = (sample_form || spec_disabled ()) ? 0 : forget_length (f);
    const int L = spec_chunk (1, W, n);
    const art_s *d_result = host_scratch.d_in;
    int rc;
    if (L) {
        const size_t need = arthip_biquad_spec_scratch (1, 1, n, L);
        if (need > host_scratch.spec_cap) {
            arthip_free (host_scratch.d_spec);
            host_scratch.d_spec = arthip_malloc (need + need / 2);
            host_scratch.spec_cap = host_scratch.d_spec ? need + need / 2 : 0;
        }
        rc = host_scratch.d_spec ? arthip_biquad_spec (host_scratch.d_state, 1, 1, host_scratch.d_in, 1, host_scratch.d_out, 1, n, L, W,
                                                       host_scratch.d_spec, host_scratch.d_first_bad, host_scratch.d_repairs, NULL) : -1;
        d_result = host_scratch.d_out;
    }
    else if (!sample_form && f->order == 2 && n >= 64)       /* long run of a narrow filter: the pipelined serial kernel, one channel */
        rc = arthip_biquad_order2 (host_scratch.d_state, 1, 1, host_scratch.d_in, n, 1, NULL);
    else
        rc = arthip_biquad_chain (host_scratch.d_state, 1, 1, host_scratch.d_in, n, sample_form ? -1 : 1, NULL);

    if (rc) pcm_fail ("biquad launch failed (samples left unfiltered)");
    else {
        if (by_kernel)
            arthip_copy2_by_kernel (h, d_result, sizeof (art_s) * (size_t) n, host_scratch.h_state, host_scratch.d_state, sizeof (Biquad), NULL);
        else {
            arthip_d2h (h, d_result, sizeof (art_s) * (size_t) n, NULL);
            arthip_d2h (host_scratch.h_state, host_scratch.d_state, sizeof (Biquad), NULL);
        }
        if (!arthip_sync (NULL)) {
            if (stride == 1) memcpy (buffer, h, sizeof (art_s) * (size_t) n);
            else for (int i = 0; i < n; ++i) buffer [(size_t) i * stride] = h [i];      /* only this channel's samples are written */
            *f = *host_scratch.h_state;
        }
        else pcm_fail ("biquad kernel failed (samples left unfiltered)");
    }
    pthread_mutex_unlock (&scratch_lock);
}

void biquad_apply_buffer (Biquad *f, artsample_t *buffer, int num_samples, int stride)
{
    biquad_run_host (f, buffer, num_samples, stride, 0);
}

/* One value through the section: the reference's per-sample association (biquad.c:78-102 — the highest delay first, each delay's
 * feed-forward and feedback products subtracted from one another before they join the sum), evaluated where the state lives: the
 * caller's struct, in host memory.  (Rounds 1-3 sent the struct and the sample to the GPU and back: one launch and 46 us per
 * sample for a dozen flops; runs of samples — biquad_apply_buffer, the decimator's noise shapers — stay on the device.  Compiled
 * -ffp-contract=off: the bits of the device kernels' sample form, tests/test_gpu_parity.py.) */
artsample_t biquad_apply_sample (Biquad *f, artsample_t input)
{
    art_s sum = input * f->a [0];
    int i = f->index & 3;

    for (int k = f->order > 4 ? 4 : f->order; k >= 1; --k) {
        const int d = (i - k + 1) & 3;
        sum += (f->x [d] * f->a [k]) - (f->b [k] * f->y [d]);
    }
    f->index = i = (i + 1) & 3;
    f->x [i] = input;
    f->y [i] = sum;
    return sum;
}

/* chunks the time-parallel biquad had to recompute since the process started (host-pointer calls; diagnostics) */
unsigned int artamdBiquadRepairs (void)
{
    unsigned int n = 0;
    pthread_mutex_lock (&scratch_lock);
    if (host_scratch.d_repairs) { arthip_d2h (&n, host_scratch.d_repairs, sizeof (n), NULL); arthip_sync (NULL); }
    pthread_mutex_unlock (&scratch_lock);
    return n;
}

/* ---- device-resident bank of section chains ---- */

struct artamd_biquad_bank {
    Biquad *d_sections;
    Biquad *d_sections0;                 /* the sections the bank was created from (biquadBankReset) */
    int C, S;
    int all_order2;                      /* every section is second order: hand-scheduled serial kernel */
    int warmup;                          /* time-parallel form: warm-up frames per section (0: serial kernels only) */
    art_s *d_tmp; size_t tmp_cap;        /* the call's input, moved aside (the time-parallel form is not in-place) */
    void *d_spec; size_t spec_cap;
    unsigned int *d_repairs;
    int *d_first_bad;
    void *stream;
    int device;
    /* a bank spread over several devices (biquadBankCreateMulti): ordinary banks with contiguous channel slices, each on its own
     * device and stream, + the slice of the caller's buffer each works on */
    int nshards; BiquadBank **shards; int *shard_first; void **ev_shard; void *ev_parent;
    art_s *d_slice; size_t slice_cap;
    unsigned long batch_stamp;           /* the last batch call that named this bank */
    void *d_batch; size_t batch_cap;     /* a batch call's table, when this bank leads it */
    /* biquadBankApplyClipsPlanarDevice, when this bank leads it: the table, the round's inputs set aside, the round's chunk states
     * (biquadBankFilterClipsPlanarDevice: the table and the chunk states with the items' mismatch flags; nothing is set aside) */
    void *d_clips; size_t clips_cap;
    void *d_clips_tmp; size_t clips_tmp_cap;
    void *d_clips_spec; size_t clips_spec_cap;
};

BiquadBank *biquadBankCreate (const Biquad *sections, int numChannels, int numSections)
{
    if (numChannels < 1 || numSections < 1 || numSections > 4 || arthip_device_count () < 1) {
        fprintf (stderr, "artamd: biquadBankCreate: need 1-4 sections, >=1 channel and a HIP device\n");
        return NULL;
    }
    BiquadBank *b = calloc (1, sizeof (*b));
    if (!b) return NULL;
    const size_t bytes = sizeof (Biquad) * (size_t) numChannels * numSections;
    b->C = numChannels; b->S = numSections;
    b->device = arthip_current_device ();
    b->all_order2 = numSections <= 2;
    b->warmup = spec_disabled () ? 0 : 1;
    for (int i = 0; i < numChannels * numSections; ++i) {
        if (sections [i].order != 2) b->all_order2 = 0;
        if (b->warmup) {
            /* (channels of one stream share their coefficients: the search runs once per distinct section) */
            int w = (i >= numSections && !memcmp (sections [i].b, sections [i - numSections].b, sizeof (sections [i].b)) &&
                     sections [i].order == sections [i - numSections].order) ? b->warmup : forget_length (sections + i);
            b->warmup = !w ? 0 : w > b->warmup ? w : b->warmup;
        }
    }
    b->d_sections = arthip_malloc (bytes);
    b->d_sections0 = arthip_malloc (bytes);
    b->d_repairs = arthip_malloc (sizeof (unsigned int));
    b->d_first_bad = arthip_malloc (sizeof (int) * (size_t) numChannels);
    if (!b->d_sections || !b->d_sections0 || !b->d_repairs || !b->d_first_bad || arthip_h2d (b->d_sections, sections, bytes, NULL) ||
        arthip_h2d (b->d_sections0, sections, bytes, NULL) || arthip_zero (b->d_repairs, sizeof (unsigned int), NULL) || arthip_biquad_spec_arm (b->d_first_bad, numChannels, NULL) ||
        arthip_sync (NULL)) { biquadBankFree (b); return NULL; }
    return b;
}

/* The same bank spread over the devices of artamdSetDevices () / ARTAMD_DEVICES (ARTAMD_SHARDS forces the count), the way a
 * RESAMPLE_MULTITHREADED resampler and a DECIMATE_MULTITHREADED decimator spread (channels are independent: art.c:1011-1017
 * filters them one by one): an ordinary bank when there is one device.  Results are those of the ordinary bank, bit for bit. */
BiquadBank *biquadBankCreateMulti (const Biquad *sections, int numChannels, int numSections)
{
    int devices [ART_MAX_DEVICES];
    const int home = arthip_current_device ();
    const int count = numChannels > 1 && arthip_device_count () >= 1 ? artamd_shard_plan (numChannels, home, devices) : 0;
    if (count <= 1) return biquadBankCreate (sections, numChannels, numSections);

    BiquadBank *b = calloc (1, sizeof (*b));
    if (!b) return NULL;
    b->C = numChannels; b->S = numSections; b->device = home;
    b->shards = calloc ((size_t) count, sizeof (BiquadBank *));
    b->shard_first = calloc ((size_t) count + 1, sizeof (int));
    b->ev_shard = calloc ((size_t) count, sizeof (void *));
    b->ev_parent = arthip_order_event_create ();
    int ok = b->shards && b->shard_first && b->ev_shard && b->ev_parent;
    const int base = numChannels / count, extra = numChannels % count;
    for (int s = 0; ok && s < count; ++s) {
        const int width = base + (s < extra ? 1 : 0);
        b->shard_first [s + 1] = b->shard_first [s] + width;
        arthip_set_device (devices [s]);
        b->shards [s] = biquadBankCreate (sections + (size_t) b->shard_first [s] * numSections, width, numSections);
        b->ev_shard [s] = arthip_order_event_create ();
        b->nshards = s + 1;
        ok = b->shards [s] && b->ev_shard [s] && (b->shards [s]->stream = arthip_stream_create ()) != NULL;
    }
    if (home >= 0) arthip_set_device (home);
    if (!ok) { fprintf (stderr, "artamd: biquadBankCreateMulti: allocation failed: %s\n", arthip_last_error ()); biquadBankFree (b); return NULL; }
    return b;
}

int biquadBankShardCount (BiquadBank *b) { return b->nshards; }

/* (work already enqueued on the old stream uses the bank's state and scratch: drained before the switch) */
void biquadBankSetStream (BiquadBank *b, void *stream)
{
    if (b->stream == stream) return;
    ENTER_DEVICE (b);
    arthip_sync (b->stream);
    LEAVE_DEVICE (b);
    b->stream = stream;
}

/* a sharded bank's call in either layout (pitch 0: interleaved; else the planes of biquadBankApplyPlanarDevice): every shard waits for
 * the bank's stream, pulls its channel slice of the caller's buffer (peer-to-peer when it sits on another device), filters it in its
 * own HBM and pushes it back; the bank's stream then waits for all of them */
static void bank_sharded_call (BiquadBank *b, artsample_t *d_buffer, long pitch, int numFrames)
{
    const int prev = arthip_current_device (), wps = (int)(sizeof (art_s) / 4);
    arthip_set_device (b->device);
    arthip_event_record (b->ev_parent, b->stream);
    for (int k = 0; k < b->nshards; ++k) {
        BiquadBank *sh = b->shards [k];
        const int first = b->shard_first [k], width = b->shard_first [k + 1] - first;
        const size_t need = sizeof (art_s) * (size_t) numFrames * width;
        arthip_set_device (sh->device);
        arthip_stream_wait_event (sh->stream, b->ev_parent);
        if (need > sh->slice_cap) {
            arthip_sync (sh->stream);
            arthip_free (sh->d_slice);
            sh->slice_cap = need + need / 2;
            if (!(sh->d_slice = arthip_malloc (sh->slice_cap))) {        /* (counted: this shard's channels stay unfiltered, as an ordinary bank's would) */
                sh->slice_cap = 0;
                pcm_fail ("sharded biquad bank: device allocation failed (a shard's channels left unfiltered)");
                arthip_event_record (b->ev_shard [k], sh->stream);
                continue;
            }
        }
        /* the slice as rows, dense in d_slice: a planar shard's planes, an interleaved one's frames of `width` channels */
        artsample_t *const mine = d_buffer + (pitch ? (size_t) first * pitch : (size_t) first);
        const int row = (pitch ? numFrames : width) * wps;
        const size_t rows = pitch ? (size_t) width : (size_t) numFrames, apart = (size_t)(pitch ? pitch : b->C) * wps;
        arthip_slice_copy (sh->d_slice, (size_t) row, mine, apart, row, rows, sh->stream);
        biquadBankApplyPlanarDevice (sh, sh->d_slice, pitch ? numFrames : 0, numFrames);       /* (pitch 0: the interleaved call) */
        arthip_slice_copy (mine, apart, sh->d_slice, (size_t) row, row, rows, sh->stream);
        arthip_event_record (b->ev_shard [k], sh->stream);
    }
    arthip_set_device (b->device);
    for (int k = 0; k < b->nshards; ++k) arthip_stream_wait_event (b->stream, b->ev_shard [k]);
    if (prev >= 0) arthip_set_device (prev);
}

/* Where a call's input is set aside: *lead samples into the copy buffer, its planes the returned pitch apart (the caller's pitch
 * modulo q, the samples of 16 bytes, and at least `frames`): the copy and its every plane start at the caller's address modulo 16. */
static long aside_placement (const void *base, long pitch, int frames, size_t *lead)
{
    const long q = 16 / (long) sizeof (art_s);
    *lead = (size_t)((uintptr_t) base & 15) / sizeof (art_s);
    return frames + (((pitch - frames) % q) + q) % q;
}

/* the time-parallel form's buffers, each grown by half as much again when a call needs more: d_tmp for `samples` samples (the
 * input set aside), d_spec for `need` bytes of chunk states.  0: one of them could not be had */
static int bank_spec_reserve (BiquadBank *b, size_t samples, size_t need)
{
    if (samples * sizeof (art_s) > b->tmp_cap) {
        arthip_free (b->d_tmp);
        b->tmp_cap = (samples + samples / 2) * sizeof (art_s);
        if (!(b->d_tmp = arthip_malloc (b->tmp_cap))) b->tmp_cap = 0;
    }
    if (need > b->spec_cap) {
        arthip_free (b->d_spec);
        b->spec_cap = need + need / 2;
        if (!(b->d_spec = arthip_malloc (b->spec_cap))) b->spec_cap = 0;
    }
    return b->d_tmp && b->d_spec;
}
/* ... and what a call says when it falls back to the serial kernels (no room, or a launch failed) */
static void bank_spec_unavailable (void) { fprintf (stderr, "artamd: time-parallel biquad unavailable (%s): serial kernel\n", arthip_last_error ()); }

void biquadBankApplyInterleavedDevice (BiquadBank *b, artsample_t *d_buffer, int numFrames)
{
    if (numFrames <= 0) return;
    if (b->nshards) { bank_sharded_call (b, d_buffer, 0, numFrames); return; }
    ENTER_DEVICE (b);
    const int L = spec_chunk (b->S, b->warmup, numFrames);

    if (L) {
        const size_t samples = (size_t) numFrames * b->C, need = arthip_biquad_spec_scratch (b->C, b->S, numFrames, L);
        if (bank_spec_reserve (b, samples, need)) {
            arthip_d2d (b->d_tmp, d_buffer, samples * sizeof (art_s), b->stream);
            if (!arthip_biquad_spec (b->d_sections, b->C, b->S, b->d_tmp, b->C, d_buffer, b->C, numFrames, L, b->warmup, b->d_spec, b->d_first_bad, b->d_repairs, b->stream)) {
                LEAVE_DEVICE (b);
                return;
            }
        }
        bank_spec_unavailable ();
    }
    if (b->all_order2 && numFrames >= 64)
        arthip_biquad_order2 (b->d_sections, b->C, b->S, d_buffer, numFrames, b->C, b->stream);
    else
        arthip_biquad_chain (b->d_sections, b->C, b->S, d_buffer, numFrames, b->C, b->stream);
    LEAVE_DEVICE (b);
}

/* Channels-first buffers.  The time-parallel form reads one buffer and writes another: the planes go aside into d_tmp by ONE 2-D
 * copy, dense but for up to 3 samples per plane — d_tmp's plane c starts at the caller's plane c's address modulo 16, so that the
 * kernel's 16-byte fetches (cut on d_tmp's boundaries) and its 16-byte stores (on the caller's) are the same cuts.  The serial form
 * is the batch kernel with this bank's planes as its lanes (a one-bank class). */
void biquadBankApplyPlanarDevice (BiquadBank *b, artsample_t *d_buffer, long pitch, int numFrames)
{
    if (numFrames <= 0) return;
    if (b->C == 1) pitch = 0;
    if (!pitch) { biquadBankApplyInterleavedDevice (b, d_buffer, numFrames); return; }
    if (b->nshards) { bank_sharded_call (b, d_buffer, pitch, numFrames); return; }
    const int L = spec_chunk (b->S, b->warmup, numFrames);

    if (L) {
        ENTER_DEVICE (b);
        size_t lead;
        const long dense = aside_placement (d_buffer, pitch, numFrames, &lead);
        const size_t samples = (size_t) dense * b->C + lead, need = arthip_biquad_spec_scratch (b->C, b->S, numFrames, L);
        const int done = bank_spec_reserve (b, samples, need) &&
            !arthip_copy2d (b->d_tmp + lead, (size_t) dense * sizeof (art_s), d_buffer, (size_t) pitch * sizeof (art_s),
                            (size_t) numFrames * sizeof (art_s), (size_t) b->C, b->stream) &&
            !arthip_biquad_spec_planar (b->d_sections, b->C, b->S, b->d_tmp + lead, dense, d_buffer, pitch, numFrames, L, b->warmup, b->d_spec,
                                        b->d_first_bad, b->d_repairs, b->stream);
        LEAVE_DEVICE (b);
        if (done) return;
        bank_spec_unavailable ();
    }
    artamd_biquad_batch_planar (&b, 1, &d_buffer, &pitch, &numFrames, 0, INT_MAX);       /* (INT_MAX: never handed back to this call) */
}

/* every section as biquadBankCreate was given it: a copy on the device, in stream order */
void biquadBankReset (BiquadBank *b)
{
    if (b->nshards) {
        for (int k = 0; k < b->nshards; ++k) biquadBankReset (b->shards [k]);
        return;
    }
    ENTER_DEVICE (b);
    if (arthip_d2d (b->d_sections, b->d_sections0, sizeof (Biquad) * (size_t) b->C * b->S, b->stream)) pcm_fail ("biquadBankReset: the copy failed (state kept)");
    LEAVE_DEVICE (b);
}

void biquadBankRead (BiquadBank *b, Biquad *sections)
{
    ENTER_DEVICE (b);
    if (b->nshards) {
        arthip_sync (b->stream);
        for (int k = 0; k < b->nshards; ++k) biquadBankRead (b->shards [k], sections + (size_t) b->shard_first [k] * b->S);
    }
    else {
        arthip_d2h (sections, b->d_sections, sizeof (Biquad) * (size_t) b->C * b->S, b->stream);
        arthip_sync (b->stream);
    }
    LEAVE_DEVICE (b);
}

/* chunks the time-parallel form had to recompute for this bank so far (synchronises; diagnostics) */
unsigned int biquadBankRepairs (BiquadBank *b)
{
    unsigned int n = 0;
    ENTER_DEVICE (b);
    if (b->nshards) {
        arthip_sync (b->stream);
        for (int k = 0; k < b->nshards; ++k) n += biquadBankRepairs (b->shards [k]);
    }
    else {
        arthip_d2h (&n, b->d_repairs, sizeof (n), b->stream);
        arthip_sync (b->stream);
    }
    LEAVE_DEVICE (b);
    return n;
}

void biquadBankFree (BiquadBank *b)
{
    if (!b) return;
    ENTER_DEVICE (b);
    arthip_sync (b->stream);
    for (int k = 0; k < b->nshards; ++k) {
        if (b->shards [k]) { void *st = b->shards [k]->stream; biquadBankFree (b->shards [k]); arthip_stream_destroy (st); }
        if (b->ev_shard && b->ev_shard [k]) arthip_event_destroy (b->ev_shard [k]);
    }
    if (b->ev_parent) arthip_event_destroy (b->ev_parent);
    free (b->shards); free (b->shard_first); free (b->ev_shard);
    arthip_free (b->d_sections); arthip_free (b->d_sections0); arthip_free (b->d_tmp); arthip_free (b->d_spec); arthip_free (b->d_repairs); arthip_free (b->d_first_bad); arthip_free (b->d_slice);
    arthip_free (b->d_batch); arthip_free (b->d_clips); arthip_free (b->d_clips_tmp); arthip_free (b->d_clips_spec);
    LEAVE_DEVICE (b);
    free (b);
}

/* ------------------------------------------------------------------------------------------
 * Decimator
 * ---------------------------------------------------------------------------------------- */

struct artamd_decimator {
    void *stream;
    /* the state the kernels carry — clip counter, error feedback, dither generators (two copies: the parallel kernel leaves
     * the advanced state in the other one), noise shapers — lives in ONE device block, so that a host-pointer call brings
     * it back in the same launch as its output; the pointers below point into it */
    unsigned char *d_state, *h_state; size_t state_bytes;          /* h_state: page-locked mirror */
    art_s *d_feedback; uint32_t *d_gens, *d_gens_alt; Biquad *d_shapers;
    unsigned long long *d_clipped;
    unsigned long long clipped_seen;
    art_s *d_in; size_t in_cap;
    unsigned char *d_out; size_t out_cap;
    unsigned char *h_in, *h_out; size_t h_in_cap, h_out_cap;       /* page-locked staging of small host-pointer calls */
    int device;                                                    /* where the state lives (and where device-pointer buffers are expected) */
    /* DECIMATE_MULTITHREADED over several devices (or ARTAMD_SHARDS): the reference's one-worker-per-channel fan-out
     * (decimator.c:92-93, 119-136) with GPUs for threads — `nshards` ordinary contexts with contiguous channel slices, each on
     * its own device and stream; this context then owns no kernel state itself, only the host mirrors of all channels */
    int nshards; Decimate **shards; int *shard_first; void **ev_shard; void *ev_parent;
    unsigned long batch_stamp;                                     /* the last batch call that named this context */
    void *d_batch; size_t batch_cap;                               /* a batch call's table, when this context leads it */
    unsigned char *d_state0;                                       /* the state block as decimateInit left it (decimateHipReset copies it back) */
    int rate, first_channel;                                       /* what the host mirrors were made from */
};
#define DEC_KERNEL_COPY_LIMIT ((size_t) 1 << 20)

/* noise-shaping transfer function N(z) (a0 == 1) -> error-feedback filter H(z), reference decimator.c:389-409 */
static void shaper_design (Biquad *f, double a1, double a2, double a3, double a4, double b1, double b2, double b3, double b4)
{
    BiquadCoefficients c;
    memset (&c, 0, sizeof (c));
    c.a0 = (art_s)(b1 - a1); c.a1 = (art_s)(b2 - a2); c.a2 = (art_s)(b3 - a3); c.a3 = (art_s)(b4 - a4);
    c.b1 = (art_s) b1; c.b2 = (art_s) b2; c.b3 = (art_s) b3; c.b4 = (art_s) b4;
    biquad_init (f, &c, 1.0);
}

static void shaper_for (Biquad *f, int flags, int rate)
{
    if (flags & SHAPING_ATH_CURVE) {
        switch (rate) {     /* ATH-curve shapers (coefficients are data of the reference, decimator.c:68-78) */
            case 32000: shaper_design (f, -0.780459, +0.569358, -0.348221, +0.466316, +0.950797, +0.282052, +0.004337, +1.76209e-5); return;
            case 44100: shaper_design (f, -1.1474, 0.5383, -0.3530, 0.3475, 1.0587, 0.0676, -0.6054, -0.2738); return;
            case 48000: shaper_design (f, -1.3344, 0.7455, -0.4602, 0.4363, 0.9030, 0.0116, -0.5853, -0.2571); return;
            case 88200: shaper_design (f, -2.150679, +2.1402057, -1.042712, +0.206838, +0.67433, +1.017047, +0.4028633, +0.098656); return;
            case 96000: shaper_design (f, -2.16994, +2.01986, -0.894857, +0.1557738, +0.517789, +1.1062189, +0.4825786, +0.244994); return;
            default:    shaper_design (f, -1.0, 0, 0, 0, 0, 0, 0, 0); return;
        }
    }
    if (flags & SHAPING_1ST_ORDER) shaper_design (f, -1.0, 0, 0, 0, 0, 0, 0, 0);
    else if (flags & SHAPING_2ND_ORDER) shaper_design (f, -2.0, +1.0, 0, 0, 0, 0, 0, 0);
    else if (flags & SHAPING_3RD_ORDER) shaper_design (f, -3.0, +3.0, -1.0, 0, 0, 0, 0, 0);
}

static uint32_t lcg_step (uint32_t r) { return ((r << 4) - r) ^ 1; }

/* the host-visible state of a fresh leaf context: feedback zero, the generators' seeds, the shapers' empty histories */
static void dec_fresh_mirrors (Decimate *cxt)
{
    const int C = cxt->numChannels;
    memset (cxt->feedback, 0, sizeof (art_s) * (size_t) C);
    if (cxt->tpdf_generators) {
        /* per-channel seeds: little-endian words cut from the byte stream (state >> 24), three steps per byte */
        uint32_t s = 0x31415926;
        memset (cxt->tpdf_generators, 0, sizeof (uint32_t) * (size_t) C);
        for (int c = -cxt->hip->first_channel; c < C; ++c)
            for (int b = 0; b < 4; ++b) {
                if (c >= 0) cxt->tpdf_generators [c] |= (uint32_t)(s >> 24) << (8 * b);
                s = lcg_step (lcg_step (lcg_step (s)));
            }
    }
    if (cxt->noise_shapers)
        for (int c = 0; c < C; ++c)
            shaper_for (cxt->noise_shapers + c, cxt->flags, cxt->hip->rate);
}

/* an ordinary context on the current device; `firstChannel`: its channels are channels firstChannel.. of a wider stream (the
 * dither generators of a stream are seeded channel after channel from one byte stream, decimator.c:40-52) */
static Decimate *dec_init_leaf (int numChannels, int outputBits, int outputBytes, double outputGain, int sampleRate, int flags, int firstChannel)
{
    Decimate *cxt = calloc (1, sizeof (Decimate));
    struct artamd_decimator *hip = calloc (1, sizeof (*hip));
    const int C = numChannels;

    if (!cxt || !hip) { free (cxt); free (hip); return NULL; }
    cxt->hip = hip;
    hip->device = arthip_current_device ();
    hip->rate = sampleRate; hip->first_channel = firstChannel;
    cxt->numChannels = C; cxt->outputBits = outputBits; cxt->outputBytes = outputBytes;
    cxt->outputGain = outputGain; cxt->flags = flags;
    cxt->feedback = calloc (C, sizeof (art_s));
    {   /* layout of the state block (every part 16-byte aligned) */
        size_t off = 16;                                                    /* [0] the clip counter */
        const size_t o_fb = off;     off += (sizeof (art_s) * C + 15) & ~(size_t) 15;
        const size_t o_g0 = off;     off += (sizeof (uint32_t) * C + 15) & ~(size_t) 15;
        const size_t o_g1 = off;     off += (sizeof (uint32_t) * C + 15) & ~(size_t) 15;
        const size_t o_sh = off;     off += (sizeof (Biquad) * C + 15) & ~(size_t) 15;
        hip->state_bytes = off;
        hip->d_state = arthip_malloc (off);
        hip->d_state0 = arthip_malloc (off);
        hip->h_state = arthip_host_alloc (off);
        if (hip->d_state && hip->d_state0 && hip->h_state) {
            arthip_zero (hip->d_state, off, NULL);
            hip->d_clipped = (unsigned long long *) hip->d_state;
            hip->d_feedback = (art_s *)(hip->d_state + o_fb);
            if (flags & DITHER_ENABLED) { hip->d_gens = (uint32_t *)(hip->d_state + o_g0); hip->d_gens_alt = (uint32_t *)(hip->d_state + o_g1); }
            if (flags & SHAPING_ENABLED) hip->d_shapers = (Biquad *)(hip->d_state + o_sh);
        }
    }

    if ((flags & DITHER_ENABLED) && hip->d_gens) {
        cxt->tpdf_generators = calloc (C, sizeof (uint32_t));
        cxt->dither_type = (flags & DITHER_HIGHPASS) ? -1 : (flags & DITHER_LOWPASS) ? 1 : 0;
    }
    if ((flags & SHAPING_ENABLED) && hip->d_shapers) cxt->noise_shapers = calloc (C, sizeof (Biquad));
    if (cxt->feedback) dec_fresh_mirrors (cxt);
    if (cxt->tpdf_generators) arthip_h2d (hip->d_gens, cxt->tpdf_generators, sizeof (uint32_t) * C, NULL);
    if (cxt->noise_shapers) arthip_h2d (hip->d_shapers, cxt->noise_shapers, sizeof (Biquad) * C, NULL);
    if (hip->d_feedback) arthip_d2d (hip->d_state0, hip->d_state, hip->state_bytes, NULL);       /* what decimateHipReset restores */

    if (arthip_sync (NULL) || !hip->d_feedback || !hip->d_clipped) {
        fprintf (stderr, "artamd: decimateInit: device setup failed: %s\n", arthip_last_error ());
        decimateFree (cxt);
        return NULL;
    }

    return cxt;
}

static Decimate *dec_init_sharded (int numChannels, int outputBits, int outputBytes, double outputGain, int sampleRate, int flags, int count, const int *devices)
{
    Decimate *cxt = calloc (1, sizeof (Decimate));
    struct artamd_decimator *hip = calloc (1, sizeof (*hip));
    const int prev = arthip_current_device (), C = numChannels;

    if (!cxt || !hip) { free (cxt); free (hip); return NULL; }
    cxt->hip = hip;
    hip->device = prev;
    cxt->numChannels = C; cxt->outputBits = outputBits; cxt->outputBytes = outputBytes;
    cxt->outputGain = outputGain; cxt->flags = flags;
    cxt->dither_type = (flags & DITHER_HIGHPASS) ? -1 : (flags & DITHER_LOWPASS) ? 1 : 0;
    cxt->feedback = calloc (C, sizeof (art_s));
    if (flags & DITHER_ENABLED) cxt->tpdf_generators = calloc (C, sizeof (uint32_t));
    if (flags & SHAPING_ENABLED) cxt->noise_shapers = calloc (C, sizeof (Biquad));
    hip->shards = calloc ((size_t) count, sizeof (Decimate *));
    hip->shard_first = calloc ((size_t) count + 1, sizeof (int));
    hip->ev_shard = calloc ((size_t) count, sizeof (void *));
    hip->ev_parent = arthip_order_event_create ();
    int ok = cxt->feedback && hip->shards && hip->shard_first && hip->ev_shard && hip->ev_parent;

    /* contiguous, balanced channel slices: the first (channels % count) shards get one channel more */
    const int base = C / count, extra = C % count;
    for (int s = 0; ok && s < count; ++s) {
        const int width = base + (s < extra ? 1 : 0);
        hip->shard_first [s + 1] = hip->shard_first [s] + width;
        arthip_set_device (devices [s]);                  /* (artamd_shard_plan has made sure it can address `prev`'s memory) */
        Decimate *leaf = dec_init_leaf (width, outputBits, outputBytes, outputGain, sampleRate, flags & ~DECIMATE_MULTITHREADED, hip->shard_first [s]);
        hip->shards [s] = leaf;
        hip->ev_shard [s] = arthip_order_event_create ();
        hip->nshards = s + 1;
        ok = leaf && hip->ev_shard [s] && (leaf->hip->stream = arthip_stream_create ()) != NULL;
        if (ok) {       /* the host-visible state of the whole stream, as every context shows it */
            const int first = hip->shard_first [s];
            if (cxt->tpdf_generators && leaf->tpdf_generators) memcpy (cxt->tpdf_generators + first, leaf->tpdf_generators, sizeof (uint32_t) * width);
            if (cxt->noise_shapers && leaf->noise_shapers) memcpy (cxt->noise_shapers + first, leaf->noise_shapers, sizeof (Biquad) * width);
        }
    }
    if (prev >= 0) arthip_set_device (prev);
    if (!ok) {
        fprintf (stderr, "artamd: sharded decimator: allocation failed: %s\n", arthip_last_error ());
        decimateFree (cxt);
        return NULL;
    }
    return cxt;
}

Decimate *decimateInit (int numChannels, int outputBits, int outputBytes, double outputGain, int sampleRate, int flags)
{
    if (numChannels < 1 || outputBits < 1 || outputBits > 24 || outputBytes < (outputBits + 7) / 8 || outputBytes > 4) {
        fprintf (stderr, "artamd: decimateInit: unsupported channel/bit/byte combination\n");
        return NULL;
    }
    if (arthip_device_count () < 1) {
        fprintf (stderr, "artamd: no usable HIP device (this library has no CPU path): %s\n", arthip_last_error ());
        return NULL;
    }
    if ((flags & DECIMATE_MULTITHREADED) && numChannels > 1) {
        int devices [ART_MAX_DEVICES];
        const int count = artamd_shard_plan (numChannels, arthip_current_device (), devices);
        if (count > 1)
            return dec_init_sharded (numChannels, outputBits, outputBytes, outputGain, sampleRate, flags, count, devices);
    }
    return dec_init_leaf (numChannels, outputBits, outputBytes, outputGain, sampleRate, flags, 0);
}

void decimateFree (Decimate *cxt)
{
    if (!cxt) return;
    struct artamd_decimator *hip = cxt->hip;
    if (hip) {
        ENTER_DEVICE (hip);
        arthip_sync (hip->stream);
        arthip_free (hip->d_state); arthip_free (hip->d_state0); arthip_host_free (hip->h_state);
        arthip_free (hip->d_in); arthip_free (hip->d_out); arthip_host_free (hip->h_in); arthip_host_free (hip->h_out);
        arthip_free (hip->d_batch);
        for (int s = 0; s < hip->nshards; ++s) {
            if (hip->shards [s]) {
                void *st = hip->shards [s]->hip ? hip->shards [s]->hip->stream : NULL;
                decimateFree (hip->shards [s]);
                arthip_stream_destroy (st);
            }
            if (hip->ev_shard && hip->ev_shard [s]) arthip_event_destroy (hip->ev_shard [s]);
        }
        if (hip->ev_parent) arthip_event_destroy (hip->ev_parent);
        free (hip->shards); free (hip->shard_first); free (hip->ev_shard);
        LEAVE_DEVICE (hip);
        free (hip);
    }
    free (cxt->feedback); free (cxt->tpdf_generators); free (cxt->noise_shapers);
    free (cxt);
}

static void dec_args (Decimate *cxt, ArtDecArgs *a)
{
    struct artamd_decimator *hip = cxt->hip;
    a->C = cxt->numChannels; a->bits = cxt->outputBits; a->bytes = cxt->outputBytes;
    a->dither_type = cxt->dither_type;
    a->dither_on = (cxt->flags & DITHER_ENABLED) != 0;
    a->shaping_on = (cxt->flags & SHAPING_ENABLED) != 0;
    a->shaping_order = (a->shaping_on && cxt->noise_shapers) ? cxt->noise_shapers [0].order : 0;
    a->scale = (art_s)((1 << cxt->outputBits) / 2.0 * cxt->outputGain);
    a->feedback = hip->d_feedback; a->gens = hip->d_gens; a->gens_next = hip->d_gens_alt; a->shapers = hip->d_shapers; a->clipped = hip->d_clipped;
}

/* (the shaper / dither state is shared between calls: the old stream is drained before the switch) */
void decimateHipSetStream (Decimate *cxt, void *stream)
{
    if (cxt->hip->stream == stream) return;
    ENTER_DEVICE (cxt->hip);
    arthip_sync (cxt->hip->stream);
    LEAVE_DEVICE (cxt->hip);
    cxt->hip->stream = stream;
}

/* shards of a DECIMATE_MULTITHREADED context (0: an ordinary context) */
int decimateHipShardCount (Decimate *cxt) { return cxt->hip->nshards; }

static void dec_swap_if (Decimate *cxt, int rc)
{
    if (rc == 1) { uint32_t *t = cxt->hip->d_gens; cxt->hip->d_gens = cxt->hip->d_gens_alt; cxt->hip->d_gens_alt = t; }
}

/* a context's staging buffers, device and page-locked, for a call of that many bytes in and out */
static int dec_reserve (Decimate *cxt, size_t in_bytes, size_t out_bytes)
{
    struct artamd_decimator *hip = cxt->hip;
    in_bytes += 16; out_bytes += 16;                    /* (copy kernels move whole words) */
    if (in_bytes > hip->in_cap) { arthip_free (hip->d_in); hip->in_cap = in_bytes * 2; if (!(hip->d_in = arthip_malloc (hip->in_cap))) { hip->in_cap = 0; return -1; } }
    if (out_bytes > hip->out_cap) { arthip_free (hip->d_out); hip->out_cap = out_bytes * 2; if (!(hip->d_out = arthip_malloc (hip->out_cap))) { hip->out_cap = 0; return -1; } }
    if (in_bytes <= DEC_KERNEL_COPY_LIMIT && in_bytes > hip->h_in_cap) {
        arthip_host_free (hip->h_in); hip->h_in_cap = in_bytes * 2;
        if (!(hip->h_in = arthip_host_alloc (hip->h_in_cap))) { hip->h_in_cap = 0; return -1; }
    }
    if (out_bytes <= DEC_KERNEL_COPY_LIMIT && out_bytes > hip->h_out_cap) {
        arthip_host_free (hip->h_out); hip->h_out_cap = out_bytes * 2;
        if (!(hip->h_out = arthip_host_alloc (hip->h_out_cap))) { hip->h_out_cap = 0; return -1; }
    }
    return 0;
}

/* a leaf context's call with a pitch on either side (0: interleaved); a one-channel context is the same call in either layout */
static void dec_leaf_pitched (Decimate *cxt, const art_s *d_input, long in_pitch, int frames, unsigned char *d_output, long out_pitch)
{
    ArtDecArgs a;
    if (cxt->numChannels == 1) in_pitch = out_pitch = 0;
    dec_args (cxt, &a);
    dec_swap_if (cxt, arthip_decimate_pitched (&a, d_input, in_pitch, frames, d_output, out_pitch, cxt->hip->stream));
}

/* a sharded context's call on device buffers (the caller's, or this context's own staging of a host-pointer call), either side
 * interleaved (pitch 0) or planar: every shard waits for the context's stream, decimates its channels with its own state, and the
 * context's stream then waits for all of them.  An interleaved side goes through the shard's staging: the shard pulls its channel
 * slice with a slice kernel (peer-to-peer when it sits on another device) and pushes its packed bytes into the interleaved output.
 * On a planar side a shard's channels are a run of the caller's planes, which it reads or writes where they lie. */
static void dec_sharded_call (Decimate *cxt, const art_s *d_input, long in_pitch, int frames, unsigned char *d_output, long out_pitch)
{
    struct artamd_decimator *hip = cxt->hip;
    const int C = cxt->numChannels, B = cxt->outputBytes, prev = arthip_current_device ();
    const int wps = (int)(sizeof (art_s) / 4);

    /* every shard's buffers first: a shard that cannot get them would leave its channels of the output unwritten, so the whole
     * call then leaves silence behind, and the failure is counted (art_hip.h: the error contract) */
    for (int k = 0; k < hip->nshards; ++k) {
        Decimate *leaf = hip->shards [k];
        const int width = hip->shard_first [k + 1] - hip->shard_first [k];
        arthip_set_device (leaf->hip->device);
        if (dec_reserve (leaf, in_pitch ? 0 : (size_t) frames * width * sizeof (art_s), out_pitch ? 0 : (size_t) frames * width * B)) {
            pcm_fail ("sharded decimator: device allocation failed (output zeroed)");
            arthip_set_device (hip->device);
            if (!out_pitch) arthip_zero (d_output, (size_t) frames * C * B, hip->stream);
            else for (int c = 0; c < C; ++c) arthip_zero (d_output + (size_t) c * out_pitch, (size_t) frames * B, hip->stream);
            if (prev >= 0) arthip_set_device (prev);
            return;
        }
    }
    arthip_set_device (hip->device);
    arthip_event_record (hip->ev_parent, hip->stream);
    for (int k = 0; k < hip->nshards; ++k) {
        Decimate *leaf = hip->shards [k];
        struct artamd_decimator *sp = leaf->hip;
        const int first = hip->shard_first [k], width = hip->shard_first [k + 1] - first;
        arthip_set_device (sp->device);
        arthip_stream_wait_event (sp->stream, hip->ev_parent);
        if (!in_pitch) arthip_slice_copy (sp->d_in, (size_t) width * wps, d_input + first, (size_t) C * wps, width * wps, (size_t) frames, sp->stream);
        dec_leaf_pitched (leaf, in_pitch ? d_input + (size_t) first * in_pitch : sp->d_in, in_pitch, frames,
                          out_pitch ? d_output + (size_t) first * out_pitch : sp->d_out, out_pitch);
        if (!out_pitch) arthip_slice_copy_bytes (d_output + (size_t) first * B, (size_t) C * B, sp->d_out, (size_t) width * B, width * B, (size_t) frames, sp->stream);
        arthip_event_record (hip->ev_shard [k], sp->stream);
    }
    arthip_set_device (hip->device);
    for (int k = 0; k < hip->nshards; ++k)
        arthip_stream_wait_event (hip->stream, hip->ev_shard [k]);
    if (prev >= 0) arthip_set_device (prev);
}

void decimateProcessInterleavedLEDevice (Decimate *cxt, const artsample_t *d_input, int numInputFrames, unsigned char *d_output)
{
    if (numInputFrames <= 0) return;
    if (cxt->hip->nshards) { dec_sharded_call (cxt, d_input, 0, numInputFrames, d_output, 0); return; }
    ArtDecArgs a;
    ENTER_DEVICE (cxt->hip);
    dec_args (cxt, &a);
    dec_swap_if (cxt, arthip_decimate (&a, d_input, numInputFrames, d_output, cxt->hip->stream));
    LEAVE_DEVICE (cxt->hip);
}

void decimateProcessPlanarLEDevice (Decimate *cxt, const artsample_t *d_input, long inputPitch, int numInputFrames,
                                    unsigned char *d_output, long outputPitch)
{
    if (numInputFrames <= 0) return;
    if (cxt->numChannels == 1) inputPitch = outputPitch = 0;
    if (!inputPitch && !outputPitch) { decimateProcessInterleavedLEDevice (cxt, d_input, numInputFrames, d_output); return; }
    if (cxt->hip->nshards) { dec_sharded_call (cxt, d_input, inputPitch, numInputFrames, d_output, outputPitch); return; }
    ENTER_DEVICE (cxt->hip);
    dec_leaf_pitched (cxt, d_input, inputPitch, numInputFrames, d_output, outputPitch);
    LEAVE_DEVICE (cxt->hip);
}

/* back to what decimateInit left, on the context's stream: the device state block from its image (all but the clip counter, which
 * counts since init), the host mirrors recomputed */
void decimateHipReset (Decimate *cxt)
{
    struct artamd_decimator *hip = cxt->hip;
    if (hip->nshards) {
        const int prev = arthip_current_device ();
        for (int k = 0; k < hip->nshards; ++k) {
            Decimate *leaf = hip->shards [k];
            const int first = hip->shard_first [k], width = hip->shard_first [k + 1] - first;
            decimateHipReset (leaf);            /* (on the shard's own stream, behind the shard's part of every earlier call) */
            if (cxt->tpdf_generators && leaf->tpdf_generators) memcpy (cxt->tpdf_generators + first, leaf->tpdf_generators, sizeof (uint32_t) * width);
            if (cxt->noise_shapers && leaf->noise_shapers) memcpy (cxt->noise_shapers + first, leaf->noise_shapers, sizeof (Biquad) * width);
        }
        memset (cxt->feedback, 0, sizeof (art_s) * (size_t) cxt->numChannels);
        if (prev >= 0) arthip_set_device (prev);
        return;
    }
    ENTER_DEVICE (hip);
    if (arthip_d2d (hip->d_state + 16, hip->d_state0 + 16, hip->state_bytes - 16, hip->stream)) pcm_fail ("decimateHipReset: the state could not be restored");
    if (hip->d_gens > hip->d_gens_alt) dec_swap_if (cxt, 1);          /* the image holds the generators in the first of the two arrays */
    LEAVE_DEVICE (hip);
    dec_fresh_mirrors (cxt);
}

/* ------------------------------------------------------------------------------------------
 * What the entries that gather many calls share (the decimator's batch / clips body, the biquad batch, clips and filter-clips
 * entries below).  Each goes route -> place -> fill -> upload -> launch: the items it cannot take are made as their single calls, the
 * others are counted into classes; every class gets a 16-byte aligned slice of ONE table, whose records are filled in place (zeroed
 * memory: a record built elsewhere and copied in would bring its padding bytes along); every present class is launched from its slice.
 * ---------------------------------------------------------------------------------------- */

/* a call can go into launches on `lead`'s stream: an ordinary bank (context) on the same stream and device */
static int bank_shares_launch (const BiquadBank *b, const BiquadBank *lead) { return !b->nshards && b->stream == lead->stream && b->device == lead->device; }
static int dec_shares_launch (const struct artamd_decimator *hip, const struct artamd_decimator *lead) { return !hip->nshards && hip->stream == lead->stream && hip->device == lead->device; }

/* item i's pitch on a side: 0 (interleaved) without a list, and for one channel (the same call in either layout) */
static long item_pitch (const long *pitches, int i, int C) { return pitches && C > 1 ? pitches [i] : 0; }

/* one side of a lane, channel c of an item of C channels: where it starts, in the units the side's pitch is counted in (a sample is
 * `width` of them), and the frames between its samples */
typedef struct { long offset; int stride; } LaneSide;
static inline LaneSide lane_side (long pitch, int c, int C, int width) { const LaneSide s = { pitch ? c * pitch : (long) c * width, pitch ? 1 : C }; return s; }

/* the next slice of a table that holds *bytes so far, for `count` records of `size` bytes: its offset; *bytes moves on to the next 16 */
static size_t table_slice (size_t *bytes, size_t size, size_t count) { const size_t at = *bytes; *bytes += (size * count + 15) & ~(size_t) 15; return at; }

/* ... and a serial class's, which holds s->count lanes: `lanes` per workgroup when forced (the measurements of the rules; 64 at most),
 * else what `rule` gives the class; the count goes up to whole workgroups (empty lanes), *maxlanes to the most of any class */
static void serial_slice (ArtBatchSlice *s, int lanes, int (*rule) (int), size_t lane_size, size_t *bytes, int *maxlanes)
{
    s->lanes = lanes > 0 ? (lanes < 64 ? lanes : 64) : rule (s->count);
    s->count = (s->count + s->lanes - 1) / s->lanes * s->lanes;
    if (s->count > *maxlanes) *maxlanes = s->count;
    s->offset = table_slice (bytes, lane_size, (size_t) s->count);
}

typedef struct { int item, channel, frames; } LaneRef;
static int lane_order (const void *pa, const void *pb)     /* longest first; then list order, channel order (a total order) */
{
    const LaneRef *a = pa, *b = pb;
    if (a->frames != b->frames) return a->frames > b->frames ? -1 : 1;
    if (a->item != b->item) return a->item < b->item ? -1 : 1;
    return a->channel < b->channel ? -1 : a->channel > b->channel;
}

/* every channel of every item of class k (cls_of [i] == k; channels_of (items [i]) of them, frames [i] long), in that order; their number */
static int bank_channels (const void *bank) { return ((const BiquadBank *) bank)->C; }
static int dec_channels (const void *cxt) { return ((const Decimate *) cxt)->numChannels; }
static int class_lanes (LaneRef *refs, int k, int n, const int *cls_of, const void *const *items, int (*channels_of) (const void *item), const int *frames)
{
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (cls_of [i] == k)
            for (int c = 0, C = channels_of (items [i]); c < C; ++c) { refs [m].item = i; refs [m].channel = c; refs [m].frames = frames [i]; ++m; }
    qsort (refs, (size_t) m, sizeof (LaneRef), lane_order);
    return m;
}

/* one strided copy of a grouped copy launch (arthip_copy_rows_launch) and the tasks a row of `width` words takes */
static long copy_groups (long width) { return (width + 3) / 4 + 1; }
static void clip_copy_item (ArtCopyRows *it, const void *src, long src_pitch, void *dst, long dst_pitch, long width, long rows, long task0)
{
    it->src = src; it->dst = dst; it->src_pitch = src_pitch; it->dst_pitch = dst_pitch;
    it->width = width; it->rows = rows; it->groups = copy_groups (width); it->task0 = task0;
}

/* The tail.  The finished table goes up to the leading item's buffer for it on `stream`: the buffer is grown first (cap NULL: it has
 * been, with the entry's scratch, whose addresses the fill needed).  0, or -1 with `failure` reported */
static int table_to_device (const char *failure, const void *table, size_t bytes, void **d_table, size_t *cap, void *stream)
{
    if (cap) *d_table = arthip_grow (*d_table, cap, bytes);
    if (*d_table && !arthip_table_upload (table, bytes, *d_table, stream)) return 0;
    pcm_fail (failure);
    return -1;
}
/* ... and a launch's result goes into the entry's tally: 0 and `made` launches more, or -1 with `failure` reported (the loops over the classes stay with the entries) */
static int launched (int failed, const char *failure, int made, int *launches) { if (failed) pcm_fail (failure); else *launches += made; return failed ? -1 : 0; }

/* ------------------------------------------------------------------------------------------
 * Many contexts, one launch per class of work
 *
 * Classes: the time-parallel form (no noise shaping, >= 64 frames: the single call's decimate_parallel_kernel), by dither on or
 * off; everything else by (shaper order, dither on or off), one lane of the serial wave per channel.  A class's lanes are sorted
 * by frame count (a workgroup runs until its longest lane ends) and cut into workgroups of arthip_decimate_batch_lanes () lanes.
 * ---------------------------------------------------------------------------------------- */
#define DEC_BATCH_CLASSES 12                       /* 2 time-parallel + 5 orders x 2 */
#define DEC_ONLY_PUT_BACK (-2)                     /* for a class: no frames, fromStart — the one grouped copy of such contexts restores it */

static unsigned long *dec_stamp (const void *cxt) { return &((const Decimate *) cxt)->hip->batch_stamp; }

/* a context's state as decimateHipReset leaves it, host side only (the device side is the caller's: the gathered launches read
 * the image): the generators live in the first of the two arrays, the mirrors are fresh */
static void dec_host_from_start (Decimate *cxt)
{
    if (cxt->hip->d_gens > cxt->hip->d_gens_alt) dec_swap_if (cxt, 1);
    dec_fresh_mirrors (cxt);
}

/* where a record's first state is read from: the live state itself, or with fromStart where the image (d_state0) of `image` holds it */
static const void *dec_first_state (const struct artamd_decimator *image, const void *live) { return live && image ? image->d_state0 + ((const unsigned char *) live - image->d_state) : live; }
/* an item's plan: its kernel arguments, its pitches (0: that side interleaved) and, for its records, the context whose image holds
 * its first state (dec_first_state's) and where its clipped samples are counted (its entry of d_clipCounts, or NULL) */
typedef struct { ArtDecArgs a; long in_pitch, out_pitch; const struct artamd_decimator *image; unsigned long long *item_clipped; } DecPlan;
/* the tasks of a context's call in a time-parallel launch */
static long dec_tasks (int C, int frames) { return (long) C * ((frames + ART_DEC_SEG - 1) / ART_DEC_SEG); }

/* route: a context that `lead`'s launches cannot take makes its single call, after its own reset with fromStart, and its clip count
 * goes up from the host; the launches made (0: no frames) */
static int dec_side_call (Decimate *cxt, const struct artamd_decimator *lead, const DecPlan *p, const artsample_t *d_input, int frames, unsigned char *d_output, int fromStart)
{
    if (fromStart) decimateHipReset (cxt);
    if (frames <= 0) return 0;
    const long before = p->item_clipped ? decimateHipClipped (cxt) : 0;
    decimateProcessPlanarLEDevice (cxt, d_input, p->in_pitch, frames, d_output, p->out_pitch);
    if (p->item_clipped) {         /* (synchronises: the read-backs, and the upload from this frame) */
        const unsigned long long made = (unsigned long long)(decimateHipClipped (cxt) - before);
        ENTER_DEVICE (lead);
        if (arthip_h2d (p->item_clipped, &made, sizeof (made), lead->stream) || arthip_sync (lead->stream))
            pcm_fail ("decimate clips: a clip count could not be uploaded");
        LEAVE_DEVICE (lead);
    }
    return 1;
}

/* route: the contexts these launches cannot take are made as their single calls, in list order (their number is returned); the
 * others get their arguments, their class (cls_of [i]; -1: nothing to do) and are counted into it, or into *nrestore */
static int dec_route (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const int *frames, unsigned char *const *d_outputs, int fromStart,
                      DecPlan *plan, int *cls_of, ArtDecClass *cls, int *nrestore)
{
    const struct artamd_decimator *lead = cxts [0]->hip;
    int side = 0;
    for (int i = 0; i < n; ++i) {
        cls_of [i] = -1;
        if (!dec_shares_launch (cxts [i]->hip, lead)) { side += dec_side_call (cxts [i], lead, &plan [i], d_inputs [i], frames [i], d_outputs [i], fromStart); continue; }
        if (frames [i] <= 0) { if (fromStart) { cls_of [i] = DEC_ONLY_PUT_BACK; ++*nrestore; } continue; }
        ArtDecArgs *a = &plan [i].a;
        dec_args (cxts [i], a);
        if (fromStart && a->gens > a->gens_next) { uint32_t *t = a->gens; a->gens = a->gens_next; a->gens_next = t; }       /* as dec_host_from_start will leave them */
        cls_of [i] = frames [i] >= 64 && !a->shaping_on ? (a->dither_on != 0)
                   : 2 + 2 * (a->shaping_on ? (a->shaping_order >= 1 && a->shaping_order <= 4 ? a->shaping_order : 4) : 0) + (a->dither_on != 0);
        ArtDecClass *c = &cls [cls_of [i]];
        if (plan [i].in_pitch || plan [i].out_pitch) c->pitched = 1;
        if (c->serial) c->slice.count += a->C;
        else { c->tasks += dec_tasks (a->C, frames [i]); c->slice.count++; }
    }
    return side;
}

/* place: the table's slices — the copies of the `nrestore` contexts that are only put back, then every present class's records; its bytes */
static size_t dec_layout (ArtDecClass *cls, int nrestore, int lanes, size_t lane_size, size_t task_size, int *maxlanes)
{
    size_t bytes = 0;
    table_slice (&bytes, sizeof (ArtCopyRows), (size_t) nrestore);
    for (int k = 0; k < DEC_BATCH_CLASSES; ++k)
        if (!cls [k].serial) cls [k].slice.offset = table_slice (&bytes, task_size, (size_t) cls [k].slice.count);
        else if (cls [k].slice.count) serial_slice (&cls [k].slice, lanes, arthip_decimate_batch_lanes, lane_size, &bytes, maxlanes);
    return bytes;
}

/* fill: an item's record of a time-parallel class at `rec` (clips: the clips entry's) */
static void dec_fill_task (unsigned char *rec, int clips, const DecPlan *p, const art_s *d_input, unsigned char *d_output, int frames, long task0)
{
    const ArtDecArgs *a = &p->a;
    ArtDecTask *it = clips ? &((ArtDecClipTask *) rec)->task : (ArtDecTask *) rec;
    it->in = d_input; it->out = d_output;
    it->feedback = (art_s *) dec_first_state (p->image, a->feedback); it->gens = (uint32_t *) dec_first_state (p->image, a->gens);       /* (both are only read by this form) */
    it->gens_next = a->gens_next; it->clipped = a->clipped;
    it->task0 = task0; it->scale = a->scale;
    it->C = a->C; it->frames = frames; it->bits = a->bits; it->bytes = a->bytes; it->dither_type = a->dither_type;
    it->in_pitch = p->in_pitch; it->out_pitch = p->out_pitch;
    if (clips) { ArtDecClipTask *ct = (ArtDecClipTask *) rec; ct->task0 = task0; ct->item_clipped = p->item_clipped; }
}

/* fill: channel c of an item as a lane of a serial class at `rec` */
static void dec_fill_lane (unsigned char *rec, int clips, const DecPlan *p, const art_s *d_input, unsigned char *d_output, int frames, int c)
{
    const ArtDecArgs *a = &p->a;
    ArtDecLane *l = clips ? &((ArtDecClipLane *) rec)->lane : (ArtDecLane *) rec;
    const LaneSide in = lane_side (p->in_pitch, c, a->C, 1), out = lane_side (p->out_pitch, c, a->C, a->bytes);
    l->in = d_input + in.offset; l->out = d_output + out.offset;
    l->feedback = a->feedback + c;
    l->gen = a->dither_on ? a->gens + c : NULL;
    l->shaper = a->shaping_on ? a->shapers + c : NULL;
    l->clipped = a->clipped; l->scale = a->scale;
    l->stride = in.stride; l->out_stride = out.stride; l->frames = frames; l->bits = a->bits; l->bytes = a->bytes; l->dither_type = a->dither_type;
    if (clips) {
        ArtDecClipLane *cl = (ArtDecClipLane *) rec;
        cl->feedback_from = dec_first_state (p->image, l->feedback); cl->gen_from = dec_first_state (p->image, l->gen);
        cl->shaper_from = dec_first_state (p->image, l->shaper); cl->item_clipped = p->item_clipped;
    }
}

/* launch: the grouped copy of the contexts that are only put back, then every present class; after each, what it leaves on the host side.  0 or -1 (reported) */
static int dec_launch (Decimate *const *cxts, int n, const int *cls_of, const ArtDecClass *cls, int nrestore, long restore_tasks, int fromStart,
                       const struct artamd_decimator *lead, int *launches)
{
    if (nrestore) {
        if (launched (arthip_copy_rows_launch (lead->d_batch, nrestore, restore_tasks, lead->stream), "decimate clips: launch failed", 1, launches)) return -1;
        for (int i = 0; i < n; ++i)
            if (cls_of [i] == DEC_ONLY_PUT_BACK) dec_host_from_start (cxts [i]);
    }
    for (int k = 0; k < DEC_BATCH_CLASSES; ++k) {
        if (!cls [k].slice.count) continue;
        if (launched (arthip_decimate_batch_launch (&cls [k], lead->d_batch, lead->stream), "decimate batch: launch failed", 1, launches)) return -1;
        for (int i = 0; i < n; ++i) {
            if (cls_of [i] != k) continue;
            if (fromStart) dec_host_from_start (cxts [i]);         /* the launch read the image and wrote the live state */
            if (!cls [k].serial) dec_swap_if (cxts [i], 1);        /* the time-parallel form left the generator state in gens_next */
        }
    }
    return 0;
}

/* lanes > 0: every serial class gets that many lanes per workgroup (the measurements of the rule); 0: the rule.
 * fromStart / d_clipCounts: decimateProcessClipsPlanarLEDevice (art_hip.h); with neither, the batch entries' records and kernels */
int artamd_decimate_clips_planar (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                  const int *numInputFrames, unsigned char *const *d_outputs, const long *outputPitches, int lanes,
                                  int fromStart, unsigned long long *d_clipCounts)
{
    if (n <= 0) return 0;
    if (artamd_batch_distinct ((const void *const *) cxts, n, dec_stamp, "decimate", "context")) return -1;
    const int clips = fromStart || d_clipCounts;                   /* the clips entry's records and instantiations */
    const size_t lane_size = clips ? sizeof (ArtDecClipLane) : sizeof (ArtDecLane), task_size = clips ? sizeof (ArtDecClipTask) : sizeof (ArtDecTask);
    struct artamd_decimator *lead = cxts [0]->hip;
    DecPlan *plan = malloc (sizeof (DecPlan) * (size_t) n);
    int *cls_of = malloc (sizeof (int) * (size_t) n);
    ArtDecClass cls [DEC_BATCH_CLASSES] = { { 0 } };
    LaneRef *refs = NULL; unsigned char *table = NULL;
    int launches = 0, rc = -1, nrestore = 0, maxlanes = 0;
    long restore_tasks = 0;
    if (!plan || !cls_of) { pcm_fail ("decimate batch: out of host memory"); goto out; }
    for (int k = 0; k < DEC_BATCH_CLASSES; ++k) { cls [k].serial = k >= 2; cls [k].order = k >= 2 ? (k - 2) / 2 : 0; cls [k].dither = k >= 2 ? (k - 2) & 1 : k; cls [k].clips = clips; }
    for (int i = 0; i < n; ++i) {
        plan [i].in_pitch = item_pitch (inputPitches, i, cxts [i]->numChannels); plan [i].out_pitch = item_pitch (outputPitches, i, cxts [i]->numChannels);
        plan [i].image = fromStart ? cxts [i]->hip : NULL; plan [i].item_clipped = d_clipCounts ? &d_clipCounts [i] : NULL;
    }
    if (d_clipCounts) {            /* every entry 0, in stream order before anything is counted */
        ENTER_DEVICE (lead);
        const int failed = arthip_zero (d_clipCounts, sizeof (unsigned long long) * (size_t) n, lead->stream);
        LEAVE_DEVICE (lead);
        if (failed) { pcm_fail ("decimate clips: the clip counts could not be cleared (nothing launched)"); goto out; }
        ++launches;
    }

    launches += dec_route (cxts, n, d_inputs, numInputFrames, d_outputs, fromStart, plan, cls_of, cls, &nrestore);
    const size_t bytes = dec_layout (cls, nrestore, lanes, lane_size, task_size, &maxlanes);
    if (!bytes) { rc = launches; goto out; }
    table = calloc (1, bytes);
    refs = maxlanes ? malloc (sizeof (LaneRef) * (size_t) maxlanes) : NULL;
    if (!table || (maxlanes && !refs)) { pcm_fail ("decimate batch: out of host memory"); goto out; }

    ArtCopyRows *back = (ArtCopyRows *) table;                      /* the contexts without frames: all but the clip counter, as decimateHipReset */
    for (int i = 0, left = nrestore; left; ++i) {
        if (cls_of [i] != DEC_ONLY_PUT_BACK) continue;
        const struct artamd_decimator *hip = cxts [i]->hip;
        clip_copy_item (back, hip->d_state0 + 16, 0, hip->d_state + 16, 0, (long)(hip->state_bytes - 16) / 4, 1, restore_tasks);
        restore_tasks += back++->groups; --left;
    }
    for (int k = 0; k < DEC_BATCH_CLASSES; ++k) {
        unsigned char *rec = table + cls [k].slice.offset;
        long task0 = 0;
        if (!cls [k].slice.count) continue;
        if (cls [k].serial) {
            const int m = class_lanes (refs, k, n, cls_of, (const void *const *) cxts, dec_channels, numInputFrames);
            for (int j = 0; j < m; ++j, rec += lane_size) {         /* (the padding lanes stay zero: 0 frames) */
                const int i = refs [j].item;
                dec_fill_lane (rec, clips, &plan [i], d_inputs [i], d_outputs [i], numInputFrames [i], refs [j].channel);
            }
        }
        else for (int i = 0; i < n; ++i) {
            if (cls_of [i] != k) continue;
            dec_fill_task (rec, clips, &plan [i], d_inputs [i], d_outputs [i], numInputFrames [i], task0);
            rec += task_size; task0 += dec_tasks (plan [i].a.C, numInputFrames [i]);
        }
    }

    ENTER_DEVICE (lead);
    if (!table_to_device ("decimate batch: the table could not be uploaded (nothing launched)", table, bytes, &lead->d_batch, &lead->batch_cap, lead->stream) &&
        !dec_launch (cxts, n, cls_of, cls, nrestore, restore_tasks, fromStart, lead, &launches)) rc = launches;
    LEAVE_DEVICE (lead);
out:
    free (plan); free (cls_of); free (refs); free (table);
    return rc;
}

int artamd_decimate_batch_planar (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                  const int *numInputFrames, unsigned char *const *d_outputs, const long *outputPitches, int lanes)
{
    return artamd_decimate_clips_planar (cxts, n, d_inputs, inputPitches, numInputFrames, d_outputs, outputPitches, lanes, 0, NULL);
}

int decimateProcessClipsPlanarLEDevice (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                        const int *numInputFrames, unsigned char *const *d_outputs, const long *outputPitches,
                                        int fromStart, unsigned long long *d_clipCounts)
{
    return artamd_decimate_clips_planar (cxts, n, d_inputs, inputPitches, numInputFrames, d_outputs, outputPitches, 0, fromStart != 0, d_clipCounts);
}

int artamd_decimate_batch (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const int *numInputFrames,
                           unsigned char *const *d_outputs, int lanes)
{
    return artamd_decimate_batch_planar (cxts, n, d_inputs, NULL, numInputFrames, d_outputs, NULL, lanes);
}

int decimateProcessBatchPlanarLEDevice (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                        const int *numInputFrames, unsigned char *const *d_outputs, const long *outputPitches)
{
    return artamd_decimate_batch_planar (cxts, n, d_inputs, inputPitches, numInputFrames, d_outputs, outputPitches, 0);
}

int decimateProcessBatchInterleavedLEDevice (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const int *numInputFrames,
                                             unsigned char *const *d_outputs)
{
    return artamd_decimate_batch (cxts, n, d_inputs, numInputFrames, d_outputs, 0);
}

/* ------------------------------------------------------------------------------------------
 * Many biquad banks, one launch per section count
 *
 * Every lane runs the serial form (pcm_kernels.hip, biquad_batch_pipe_kernel), whatever form the bank's single call would take:
 * all of them give the reference's bits.  Only a call that its single call would make time-parallel AND that is longer than
 * BQ_BATCH_SERIAL_MAX frames stays on the side: from there on one serial lane takes longer than that whole single call.  A class's
 * lanes are sorted by frame count and cut into workgroups of arthip_biquad_batch_lanes () lanes.
 * ---------------------------------------------------------------------------------------- */
#define BQ_BATCH_SERIAL_MAX 512                    /* measured: profiles/biquad_batch.txt (--sweep, serial_max): one serial lane of ART's
                                                    * pre-filter takes as long as its time-parallel single call at 510-570 frames */

static unsigned long *bank_stamp (const void *b) { return &((BiquadBank *) b)->batch_stamp; }

/* lanes > 0: every class gets that many lanes per workgroup; serialMax < 0: BQ_BATCH_SERIAL_MAX (the measurements of both rules) */
int artamd_biquad_batch (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const int *numFrames, int lanes, int serialMax)
{
    return artamd_biquad_batch_planar (banks, n, d_buffers, NULL, numFrames, lanes, serialMax);
}

/* place: the slices of the serial classes (section counts 1 - 4: cls [S - 1]) that have lanes, from *bytes on */
static void bq_serial_layout (ArtBqClass *cls, int lanes, size_t lane_size, size_t *bytes, int *maxlanes)
{
    for (int k = 0; k < 4; ++k)
        if (cls [k].slice.count) { cls [k].S = k + 1; serial_slice (&cls [k].slice, lanes, arthip_biquad_batch_lanes, lane_size, bytes, maxlanes); }
}

/* pitches: NULL (every item interleaved) or a pitch per item, 0 for an interleaved one (biquadBankApplyPlanarDevice's) */
int artamd_biquad_batch_planar (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const long *pitches, const int *numFrames,
                                int lanes, int serialMax)
{
    if (n <= 0) return 0;
    if (artamd_batch_distinct ((const void *const *) banks, n, bank_stamp, "biquad", "bank")) return -1;
    if (serialMax < 0) serialMax = BQ_BATCH_SERIAL_MAX;
    BiquadBank *lead = banks [0];
    int *cls_of = malloc (sizeof (int) * (size_t) n);
    ArtBqClass cls [4] = { { 0 } };
    LaneRef *refs = NULL; unsigned char *table = NULL;
    int launches = 0, rc = -1, maxlanes = 0;
    size_t bytes = 0;
    if (!cls_of) { pcm_fail ("biquad batch: out of host memory"); goto out; }
    /* route: the calls this launch cannot take are made as their single calls, in list order; the others are counted into their
     * class, cls_of [i] = S - 1 (-1: not gathered) */
    for (int i = 0; i < n; ++i) {
        BiquadBank *b = banks [i];
        cls_of [i] = -1;
        if (numFrames [i] <= 0) continue;
        if (bank_shares_launch (b, lead) && !gathered_chunk (b->S, b->warmup, numFrames [i], serialMax)) cls [cls_of [i] = b->S - 1].slice.count += b->C;
        else { biquadBankApplyPlanarDevice (b, d_buffers [i], item_pitch (pitches, i, b->C), numFrames [i]); ++launches; }       /* (pitch 0: the interleaved call) */
    }
    bq_serial_layout (cls, lanes, sizeof (ArtBqLane), &bytes, &maxlanes);
    if (!bytes) { rc = launches; goto out; }
    table = calloc (1, bytes);
    refs = malloc (sizeof (LaneRef) * (size_t) maxlanes);
    if (!table || !refs) { pcm_fail ("biquad batch: out of host memory"); goto out; }
    for (int k = 0; k < 4; ++k) {
        if (!cls [k].slice.count) continue;
        const int m = class_lanes (refs, k, n, cls_of, (const void *const *) banks, bank_channels, numFrames);
        ArtBqLane *l = (ArtBqLane *)(table + cls [k].slice.offset);         /* (the padding lanes stay zero: 0 frames) */
        for (int j = 0; j < m; ++j) {
            const int i = refs [j].item, c = refs [j].channel;
            const BiquadBank *b = banks [i];
            const LaneSide at = lane_side (item_pitch (pitches, i, b->C), c, b->C, 1);
            l [j].sections = b->d_sections + (size_t) c * b->S;
            l [j].buf = d_buffers [i] + at.offset; l [j].stride = at.stride; l [j].frames = refs [j].frames;
        }
    }

    ENTER_DEVICE (lead);
    rc = table_to_device ("biquad batch: the table could not be uploaded (nothing launched)", table, bytes, &lead->d_batch, &lead->batch_cap, lead->stream);
    for (int k = 0; k < 4 && !rc; ++k)
        if (cls [k].slice.count) rc = launched (arthip_biquad_batch_launch (&cls [k], lead->d_batch, lead->stream), "biquad batch: launch failed", 1, &launches);
    if (!rc) rc = launches;
    LEAVE_DEVICE (lead);
out:
    free (cls_of); free (refs); free (table);
    return rc;
}

int biquadBankApplyBatchInterleavedDevice (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const int *numFrames)
{
    return artamd_biquad_batch (banks, n, d_buffers, numFrames, 0, -1);
}

int biquadBankApplyBatchPlanarDevice (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const long *pitches, const int *numFrames)
{
    return artamd_biquad_batch_planar (banks, n, d_buffers, pitches, numFrames, 0, -1);
}

int artamd_biquad_batch_serial_max (void) { return BQ_BATCH_SERIAL_MAX; }

/* ------------------------------------------------------------------------------------------
 * Many banks' whole clips: the time-parallel form in shared launches
 *
 * The batch entry above leaves a long time-parallel call to its single call: four enqueues per bank, each a few waves wide.  Here
 * those calls are gathered: every item keeps the chunk length, chunk count and warm-up of its single call (so the chunk cuts, the
 * repairs and the bits are that call's), and the items of one (section count, layout) class share one spec, one check and one
 * commit launch (pcm_kernels.hip, bq_clips_spec_kernel).  One grouped copy launch sets every item's frames aside — a planar
 * item's planes at their own addresses modulo 16, as biquadBankApplyPlanarDevice places them — and, with fromStart, puts the sections
 * of the banks that do not go through the gathered launches back to their first state.  What the batch entry gathers goes to it, in one
 * call; sharded banks and banks on another stream or device are single calls, and so is a time-parallel call that is the only one of
 * its list.
 *
 * The copies and the chunk states live with banks [0], shared by the items.  Items are taken in list order in rounds whose copies
 * stay under BQ_CLIPS_ROUND_BYTES (an item beyond it is a round of its own): a round's launches are
 * 1 copy + 3 per present class, at most 1 + 3 * 8.
 * ---------------------------------------------------------------------------------------- */
#define BQ_CLIPS_ROUND_BYTES ((size_t) 128 << 20)  /* half of the 256 MiB the chip's last-level cache holds: a round's copy and the
                                                    * part of the callers' buffers it is written back to fit in it together, and
                                                    * 128 MiB is some 380 one-second stereo clips of 4-byte samples — 760 planes of
                                                    * dozens to hundreds of chunks, many waves per SIMD.  The scratch of a call stays
                                                    * under 1.5 x (this + its chunk states, at most half as much again) whatever the batch */
#define BQ_CLIP_CLASSES 8                          /* section counts 1-4 x (interleaved, planar) */

enum { CLIP_SKIP, CLIP_SIDE, CLIP_SERIAL, CLIP_GATHERED };
/* an item's route and, for a gathered one, its place: round, class, slot, first channel and first task in the class, chunk count
 * and length, and where its chunk states lie in the state buffer (bytes).  The leading part of both entries' plans */
typedef struct { int kind, round, cls, slot, chan0, K, L; long task0; size_t spec_at; } ClipPlace;
typedef struct {
    ClipPlace at;
    int copy_slot;
    long copy_task0, dense, pitch;
    size_t lead, tmp_at;                 /* samples before the first frame in its 16-byte group; of the item's first frame in the copy
                                          * buffer (samples) */
} ClipPlan;
typedef struct {
    int ncopy; long copy_tasks; size_t copy_offset;
    size_t tmp_bytes, spec_bytes;
    ArtBqClipClass cls [BQ_CLIP_CLASSES];
} ClipRound;

/* The one copy of the gathered items' bookkeeping, for this entry and the out-of-place one below.
 * clip_place: a gathered item of `frames` frames (p->L set by the route rule) takes its place in its (section count, layout) class
 * of its round's `classes`, which count on */
static void clip_place (ClipPlace *p, ArtBqClipClass *classes, const BiquadBank *b, int frames, int planar)
{
    p->K = (frames + p->L - 1) / p->L;
    ArtBqClipClass *c = &classes [p->cls = 2 * (b->S - 1) + (planar != 0)];
    c->S = b->S; c->planar = planar != 0;
    p->slot = c->count++; p->task0 = c->tasks; p->chan0 = c->channels;
    c->tasks += (long) b->C * p->K; c->channels += b->C;
}

/* the table's slices, per round its copies (the in-place entry's), then its classes' items; the bytes, and the most bytes a round
 * sets aside and keeps as chunk states */
static size_t clip_rounds_layout (ClipRound *rounds, int nrounds, size_t *tmp_need, size_t *spec_need)
{
    size_t bytes = 0;
    for (ClipRound *r = rounds; r < rounds + nrounds; ++r) {
        r->copy_offset = table_slice (&bytes, sizeof (ArtCopyRows), (size_t) r->ncopy);
        for (int k = 0; k < BQ_CLIP_CLASSES; ++k) r->cls [k].offset = table_slice (&bytes, sizeof (ArtBqClip), (size_t) r->cls [k].count);
        if (r->tmp_bytes > *tmp_need) *tmp_need = r->tmp_bytes;
        if (r->spec_bytes > *spec_need) *spec_need = r->spec_bytes;
    }
    return bytes;
}

/* a placed item's record in the table, with the fields both entries set alike; the buffers, sections and flags are the caller's */
static ArtBqClip *clip_item (unsigned char *table, const ArtBqClipClass *classes, const ClipPlace *p, const BiquadBank *b, int frames, void *states)
{
    ArtBqClip *it = (ArtBqClip *)(table + classes [p->cls].offset) + p->slot;
    it->task0 = p->task0; it->chan0 = p->chan0;
    it->C = b->C; it->K = p->K; it->L = p->L; it->W = b->warmup; it->frames = frames;
    it->states = states;
    return it;
}

/* the 4-byte words of a sample and of a bank's sections (what the grouped copy that puts a bank back moves) */
#define WORDS_PER_SAMPLE ((long)(sizeof (art_s) / 4))
static long bank_words (const BiquadBank *b) { return (long)(sizeof (Biquad) / 4) * b->C * b->S; }

/* route: every call's kind and, for a time-parallel one, its chunk length.  A lone time-parallel call gains nothing from the table
 * (measured, profiles/biquad_clips.txt: 4 us behind its single call): it is made as that call */
static void clips_route (BiquadBank *const *banks, int n, const long *pitches, const int *numFrames, ClipPlan *plan)
{
    int ngathered = 0, only = -1;
    for (int i = 0; i < n; ++i) {
        const BiquadBank *b = banks [i];
        ClipPlan *p = &plan [i];
        p->pitch = item_pitch (pitches, i, b->C);
        if (!bank_shares_launch (b, banks [0])) p->at.kind = CLIP_SIDE;
        else if ((p->at.L = gathered_chunk (b->S, b->warmup, numFrames [i], BQ_BATCH_SERIAL_MAX)) != 0) { p->at.kind = CLIP_GATHERED; ++ngathered; only = i; }
        else p->at.kind = numFrames [i] > 0 ? CLIP_SERIAL : CLIP_SKIP;
    }
    if (ngathered == 1) plan [only].at.kind = CLIP_SIDE;
}

/* place: an item's copy takes the next slot and `tasks` tasks of a round's copy launch */
static void clips_place_copy (ClipPlan *p, ClipRound *r, long tasks) { p->copy_slot = r->ncopy++; p->copy_task0 = r->copy_tasks; r->copy_tasks += tasks; }

/* place: a gathered item in the last of the `nrounds` rounds, or in a new one when its copy would take that one beyond `bound` bytes;
 * the rounds there are now.  The copy is placed as the single call's (an interleaved item's copy then moves 16 bytes at a time too) */
static int clips_place (ClipPlan *p, ClipRound *rounds, int nrounds, const BiquadBank *b, const artsample_t *d_buffer, int frames, size_t bound)
{
    const size_t q = 16 / sizeof (art_s);
    p->dense = aside_placement (d_buffer, p->pitch, frames, &p->lead);
    if (!p->pitch) p->dense = (long) frames * b->C;
    const size_t samples = ((p->pitch ? (size_t) p->dense * b->C : (size_t) p->dense) + p->lead + (q - 1)) & ~(q - 1);
    const size_t states = (arthip_biquad_spec_scratch (b->C, b->S, frames, p->at.L) + 255) & ~(size_t) 255;
    ClipRound *r = &rounds [nrounds - 1];
    if (r->tmp_bytes && r->tmp_bytes + samples * sizeof (art_s) > bound) r = &rounds [nrounds++];
    p->at.round = (int)(r - rounds);
    p->tmp_at = r->tmp_bytes / sizeof (art_s) + p->lead; r->tmp_bytes += samples * sizeof (art_s);
    p->at.spec_at = r->spec_bytes; r->spec_bytes += states;
    clip_place (&p->at, r->cls, b, frames, p->pitch != 0);
    clips_place_copy (p, r, p->pitch ? b->C * copy_groups (frames * WORDS_PER_SAMPLE) : copy_groups (p->dense * WORDS_PER_SAMPLE));
    return nrounds;
}

/* fill: a gathered item's copy aside (into the lead's d_clips_tmp) and its record, in its round `r`'s slices */
static void clips_fill_item (unsigned char *table, const ClipRound *r, const ClipPlan *p, const BiquadBank *b, artsample_t *d_buffer, int frames,
                             int fromStart, const BiquadBank *lead)
{
    art_s *const aside = (art_s *) lead->d_clips_tmp + p->tmp_at;
    ArtCopyRows *copy = (ArtCopyRows *)(table + r->copy_offset) + p->copy_slot;
    if (p->pitch) clip_copy_item (copy, d_buffer, p->pitch * WORDS_PER_SAMPLE, aside, p->dense * WORDS_PER_SAMPLE, frames * WORDS_PER_SAMPLE, b->C, p->copy_task0);
    else clip_copy_item (copy, d_buffer, 0, aside, 0, p->dense * WORDS_PER_SAMPLE, 1, p->copy_task0);
    ArtBqClip *it = clip_item (table, r->cls, &p->at, b, frames, (char *) lead->d_clips_spec + p->at.spec_at);
    it->from = fromStart ? b->d_sections0 : b->d_sections; it->sections = b->d_sections;
    it->in = aside; it->out = d_buffer;
    it->in_stride = p->pitch ? p->dense : b->C; it->out_stride = p->pitch ? p->pitch : b->C;
    it->first_bad = b->d_first_bad; it->repairs = b->d_repairs;
}

/* launch: round after round its copy launch, then its classes' from lead->d_clips; behind the first round's copy launch (their
 * sections are put back) what the batch entry gathers goes to it, in one call.  0, or -1 (reported) */
static int clips_launch (const ClipRound *rounds, int nrounds, const BiquadBank *lead, BiquadBank *const *sbanks, int nserial, artsample_t *const *sbufs,
                         const long *spitches, const int *sframes, int *launches)
{
    for (int r = 0; r < nrounds; ++r) {
        const ClipRound *rd = &rounds [r];
        if (rd->ncopy && launched (arthip_copy_rows_launch ((const char *) lead->d_clips + rd->copy_offset, rd->ncopy, rd->copy_tasks, lead->stream),
                                   "biquad clips: launch failed", 1, launches)) return -1;
        if (r == 0 && nserial) {
            const int made = artamd_biquad_batch_planar (sbanks, nserial, sbufs, spitches, sframes, 0, -1);
            if (made < 0) return -1;
            *launches += made;
        }
        for (int k = 0; k < BQ_CLIP_CLASSES; ++k)
            if (rd->cls [k].count && launched (arthip_biquad_clips_launch (&rd->cls [k], lead->d_clips, lead->stream), "biquad clips: launch failed", 3, launches)) return -1;
    }
    return 0;
}

int artamd_biquad_clips_planar (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const long *pitches, const int *numFrames,
                                int fromStart, long roundBytes)
{
    if (n <= 0) return 0;
    if (artamd_batch_distinct ((const void *const *) banks, n, bank_stamp, "biquad clips", "bank")) return -1;
    const size_t bound = roundBytes > 0 ? (size_t) roundBytes : BQ_CLIPS_ROUND_BYTES;
    BiquadBank *lead = banks [0];
    ClipPlan *plan = calloc ((size_t) n, sizeof (ClipPlan));
    ClipRound *rounds = calloc ((size_t) n + 1, sizeof (ClipRound));
    BiquadBank **sbanks = malloc (sizeof (BiquadBank *) * (size_t) n);         /* what goes to the batch entry: banks, buffers, pitches, frames */
    artsample_t **sbufs = malloc (sizeof (artsample_t *) * (size_t) n);
    long *spitches = malloc (sizeof (long) * (size_t) n);
    int *sframes = malloc (sizeof (int) * (size_t) n);
    unsigned char *table = NULL;
    int launches = 0, rc = -1, nrounds = 1, nserial = 0;
    if (!plan || !rounds || !sbanks || !sbufs || !spitches || !sframes) { pcm_fail ("biquad clips: out of host memory"); goto out; }
    clips_route (banks, n, pitches, numFrames, plan);
    /* the calls these launches cannot take are made as their single calls, in list order; the others get their places */
    for (int i = 0; i < n; ++i) {
        BiquadBank *b = banks [i];
        ClipPlan *p = &plan [i];
        const int frames = numFrames [i];
        if (p->at.kind == CLIP_SIDE) {
            if (fromStart) biquadBankReset (b);
            if (frames > 0) { biquadBankApplyPlanarDevice (b, d_buffers [i], p->pitch, frames); ++launches; }
            continue;
        }
        if (p->at.kind == CLIP_GATHERED) { nrounds = clips_place (p, rounds, nrounds, b, d_buffers [i], frames, bound); continue; }
        if (p->at.kind == CLIP_SERIAL) { sbanks [nserial] = b; sbufs [nserial] = d_buffers [i]; spitches [nserial] = p->pitch; sframes [nserial] = frames; ++nserial; }
        if (fromStart) clips_place_copy (p, &rounds [0], copy_groups (bank_words (b)));      /* its sections are put back by the first round's copy launch */
    }

    size_t tmp_need = 0, spec_need = 0;
    const size_t bytes = clip_rounds_layout (rounds, nrounds, &tmp_need, &spec_need);
    if (!bytes && !nserial) { rc = launches; goto out; }

    ENTER_DEVICE (lead);
    rc = 0;
    if (bytes) {
        table = calloc (1, bytes);
        lead->d_clips = arthip_grow (lead->d_clips, &lead->clips_cap, bytes);
        if (tmp_need) lead->d_clips_tmp = arthip_grow (lead->d_clips_tmp, &lead->clips_tmp_cap, tmp_need);
        if (spec_need) lead->d_clips_spec = arthip_grow (lead->d_clips_spec, &lead->clips_spec_cap, spec_need);
        if (!table || !lead->d_clips || (tmp_need && !lead->d_clips_tmp) || (spec_need && !lead->d_clips_spec)) {
            pcm_fail ("biquad clips: out of memory for the table or the scratch (nothing of the gathered calls launched)");
            rc = -1;
        }
    }
    for (int i = 0; i < n && !rc && bytes; ++i) {
        const ClipPlan *p = &plan [i];
        const BiquadBank *b = banks [i];
        if (p->at.kind == CLIP_GATHERED) clips_fill_item (table, &rounds [p->at.round], p, b, d_buffers [i], numFrames [i], fromStart, lead);
        else if (p->at.kind != CLIP_SIDE && fromStart)
            clip_copy_item ((ArtCopyRows *)(table + rounds [0].copy_offset) + p->copy_slot, b->d_sections0, 0, b->d_sections, 0, bank_words (b), 1, p->copy_task0);
    }
    if (!rc && bytes) rc = table_to_device ("biquad clips: the table could not be uploaded (nothing of the gathered calls launched)", table, bytes, &lead->d_clips, NULL, lead->stream);
    if (!rc) rc = clips_launch (rounds, nrounds, lead, sbanks, nserial, sbufs, spitches, sframes, &launches) ? -1 : launches;
    LEAVE_DEVICE (lead);
out:
    free (plan); free (rounds); free (sbanks); free (sbufs); free (spitches); free (sframes); free (table);
    return rc;
}

int biquadBankApplyClipsPlanarDevice (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const long *pitches, const int *numFrames,
                                      int fromStart)
{
    return artamd_biquad_clips_planar (banks, n, d_buffers, pitches, numFrames, fromStart, 0);
}

/* ------------------------------------------------------------------------------------------
 * Whole clips out of place from the banks' first state, forwards or with time reversed (biquadBankFilterClipsPlanarDevice, art_hip.h)
 *
 * The routes and the chunk cuts are the clips entry's (reversed: on the reversed sequence), but the kernels read the caller's input
 * where it lies and write the caller's output: no set-aside copy, no state stored back, nothing of a bank written.  So there is no
 * side route (a bank on another stream is only read: its first state never changes after biquadBankCreate), a lone time-parallel
 * item goes through the gathered launches, and the serial items have a kernel of their own that reads one side and writes the other.
 * Rounds are cut on the chunk-state bytes, the only scratch; each item's mismatch flags (C ints) lie behind its chunk states and
 * are armed by the speculative launch.  One table for the whole call: per round its classes' items, then the serial classes' lanes.
 * ---------------------------------------------------------------------------------------- */
typedef struct { ClipPlace at; long in_pitch, out_pitch; size_t flags_at; } FilterPlan;       /* (the rounds are ClipRounds without copies) */

/* samples from the first to behind the last one of an item's side */
static size_t filter_extent (int C, long pitch, int frames) { return pitch ? (size_t)(C - 1) * (size_t) pitch + (size_t) frames : (size_t) frames * C; }

/* the refusals: before anything is allocated or enqueued, and not counted */
static int filter_refuses (BiquadBank *const *banks, int n, const artsample_t *const *d_ins, const long *in_pitches, artsample_t *const *d_outs,
                           const long *out_pitches, const int *numFrames)
{
    for (int i = 0; i < n; ++i) {
        const BiquadBank *b = banks [i];
        if (numFrames [i] <= 0) continue;
        if (!b || !d_ins [i] || !d_outs [i] || b->nshards || b->device != banks [0]->device) return 1;
        const long ip = item_pitch (in_pitches, i, b->C), op = item_pitch (out_pitches, i, b->C);
        if (!ip != !op || ip < 0 || op < 0 || (ip && ip < numFrames [i]) || (op && op < numFrames [i])) return 1;
        const uintptr_t in0 = (uintptr_t) d_ins [i], in1 = in0 + filter_extent (b->C, ip, numFrames [i]) * sizeof (art_s);
        const uintptr_t out0 = (uintptr_t) d_outs [i], out1 = out0 + filter_extent (b->C, op, numFrames [i]) * sizeof (art_s);
        if (in0 < out1 && out0 < in1) return 1;
    }
    return banks [0]->nshards != 0;
}

/* launch: the serial classes, then round after round its classes, from lead->d_clips.  0, or -1 (reported) */
static int filter_launch (const ArtBqClass *ser, const ClipRound *rounds, int nrounds, int reversed, const BiquadBank *lead, int *launches)
{
    for (int k = 0; k < 4; ++k)
        if (ser [k].slice.count && launched (arthip_biquad_filter_batch_launch (&ser [k], lead->d_clips, reversed, lead->stream),
                                             "biquad filter clips: launch failed", 1, launches)) return -1;
    for (int r = 0; r < nrounds; ++r)
        for (int k = 0; k < BQ_CLIP_CLASSES; ++k)
            if (rounds [r].cls [k].count && launched (arthip_biquad_filter_clips_launch (&rounds [r].cls [k], lead->d_clips, reversed, lead->stream),
                                                      "biquad filter clips: launch failed", 3, launches)) return -1;
    return 0;
}

int artamd_biquad_filter_clips_planar (BiquadBank *const *banks, int n, const artsample_t *const *d_ins, const long *in_pitches,
                                       artsample_t *const *d_outs, const long *out_pitches, const int *numFrames, int reversed, long roundBytes)
{
    if (n <= 0) return 0;
    if (!banks || !banks [0] || !numFrames || !d_ins || !d_outs) return -1;
    if (filter_refuses (banks, n, d_ins, in_pitches, d_outs, out_pitches, numFrames)) return -1;
    const size_t bound = roundBytes > 0 ? (size_t) roundBytes : BQ_CLIPS_ROUND_BYTES;
    BiquadBank *lead = banks [0];
    FilterPlan *plan = calloc ((size_t) n, sizeof (FilterPlan));
    ClipRound *rounds = calloc ((size_t) n + 1, sizeof (ClipRound));
    int *ser_of = malloc (sizeof (int) * (size_t) n);                /* an item's serial class, S - 1, or -1 */
    LaneRef *refs = NULL; unsigned char *table = NULL;
    ArtBqClass ser [4] = { { 0 } };
    int launches = 0, rc = -1, nrounds = 1, maxlanes = 0;
    if (!plan || !rounds || !ser_of) { pcm_fail ("biquad filter clips: out of host memory"); goto out; }
    /* every item's route (the clips entry's rule) and place */
    for (int i = 0; i < n; ++i) {
        const BiquadBank *b = banks [i];
        FilterPlan *p = &plan [i];
        const int frames = numFrames [i];
        ser_of [i] = -1;
        if (frames <= 0) { p->at.kind = CLIP_SKIP; continue; }
        p->in_pitch = item_pitch (in_pitches, i, b->C); p->out_pitch = item_pitch (out_pitches, i, b->C);
        if ((p->at.L = gathered_chunk (b->S, b->warmup, frames, BQ_BATCH_SERIAL_MAX)) == 0) { p->at.kind = CLIP_SERIAL; ser [ser_of [i] = b->S - 1].slice.count += b->C; continue; }
        p->at.kind = CLIP_GATHERED;
        const size_t states = arthip_biquad_spec_scratch (b->C, b->S, frames, p->at.L);         /* (a multiple of 32 bytes: the flags lie aligned behind it) */
        const size_t need = (states + sizeof (int) * (size_t) b->C + 255) & ~(size_t) 255;
        ClipRound *r = &rounds [nrounds - 1];
        if (r->spec_bytes && r->spec_bytes + need > bound) r = &rounds [nrounds++];
        p->at.round = (int)(r - rounds);
        p->at.spec_at = r->spec_bytes; p->flags_at = p->at.spec_at + states; r->spec_bytes += need;
        clip_place (&p->at, r->cls, b, frames, p->in_pitch != 0);
    }

    /* the table: per round its classes' items, then the serial classes' lanes */
    size_t tmp_need = 0, spec_need = 0, bytes = clip_rounds_layout (rounds, nrounds, &tmp_need, &spec_need);
    bq_serial_layout (ser, 0, sizeof (ArtBqFilterLane), &bytes, &maxlanes);
    if (!bytes) { rc = 0; goto out; }
    table = calloc (1, bytes);
    refs = malloc (sizeof (LaneRef) * (size_t)(maxlanes ? maxlanes : 1));
    if (!table || !refs) { pcm_fail ("biquad filter clips: out of host memory"); goto out; }

    ENTER_DEVICE (lead);
    rc = 0;
    lead->d_clips = arthip_grow (lead->d_clips, &lead->clips_cap, bytes);
    if (spec_need) lead->d_clips_spec = arthip_grow (lead->d_clips_spec, &lead->clips_spec_cap, spec_need);
    if (!lead->d_clips || (spec_need && !lead->d_clips_spec)) {
        pcm_fail ("biquad filter clips: out of memory for the table or the chunk states (nothing launched)");
        rc = -1;
    }
    for (int i = 0; i < n && !rc; ++i) {         /* the gathered items: chunk states and, behind them, flags in the lead's d_clips_spec */
        const FilterPlan *p = &plan [i];
        const BiquadBank *b = banks [i];
        if (p->at.kind != CLIP_GATHERED) continue;
        ArtBqClip *it = clip_item (table, rounds [p->at.round].cls, &p->at, b, numFrames [i], (char *) lead->d_clips_spec + p->at.spec_at);
        it->from = b->d_sections0; it->sections = NULL;
        it->in = d_ins [i]; it->out = d_outs [i];
        it->in_stride = p->in_pitch ? p->in_pitch : b->C; it->out_stride = p->out_pitch ? p->out_pitch : b->C;
        it->first_bad = (int *)((char *) lead->d_clips_spec + p->flags_at); it->repairs = lead->d_repairs;
    }
    for (int k = 0; k < 4 && !rc; ++k) {
        if (!ser [k].slice.count) continue;
        const int m = class_lanes (refs, k, n, ser_of, (const void *const *) banks, bank_channels, numFrames);
        ArtBqFilterLane *l = (ArtBqFilterLane *)(table + ser [k].slice.offset);      /* (the padding lanes stay zero: 0 frames) */
        for (int j = 0; j < m; ++j) {
            const int i = refs [j].item, c = refs [j].channel, C = banks [i]->C;
            const LaneSide in = lane_side (plan [i].in_pitch, c, C, 1), out = lane_side (plan [i].out_pitch, c, C, 1);
            l [j].sections = banks [i]->d_sections0 + (size_t) c * banks [i]->S;
            l [j].in = d_ins [i] + in.offset; l [j].out = d_outs [i] + out.offset;
            l [j].in_stride = in.stride; l [j].out_stride = out.stride; l [j].frames = refs [j].frames;
        }
    }
    if (!rc) rc = table_to_device ("biquad filter clips: the table could not be uploaded (nothing launched)", table, bytes, &lead->d_clips, NULL, lead->stream);
    if (!rc) rc = filter_launch (ser, rounds, nrounds, reversed != 0, lead, &launches) ? -1 : launches;
    LEAVE_DEVICE (lead);
out:
    free (plan); free (rounds); free (ser_of); free (refs); free (table);
    return rc;
}

int biquadBankFilterClipsPlanarDevice (BiquadBank *const *banks, int n, const artsample_t *const *d_ins, const long *in_pitches,
                                       artsample_t *const *d_outs, const long *out_pitches, const int *numFrames, int reversed)
{
    return artamd_biquad_filter_clips_planar (banks, n, d_ins, in_pitches, d_outs, out_pitches, numFrames, reversed, 0);
}

long decimateHipClipped (Decimate *cxt)
{
    unsigned long long total = 0;
    if (cxt->hip->nshards) {
        long sum = 0;
        {
            ENTER_DEVICE (cxt->hip);
            arthip_sync (cxt->hip->stream);
            LEAVE_DEVICE (cxt->hip);
        }
        for (int k = 0; k < cxt->hip->nshards; ++k) sum += decimateHipClipped (cxt->hip->shards [k]);
        return sum;
    }
    ENTER_DEVICE (cxt->hip);
    arthip_d2h (&total, cxt->hip->d_clipped, sizeof (total), cxt->hip->stream);
    arthip_sync (cxt->hip->stream);
    LEAVE_DEVICE (cxt->hip);
    return (long) total;
}

/* after a host-pointer call: bring back the output (out_bytes from d_out; NULL destination: the caller fetched it itself)
 * together with the state block, return this call's clip count and refresh the host-visible state mirrors */
static int dec_finish (Decimate *cxt, unsigned char *output, size_t out_bytes)
{
    struct artamd_decimator *hip = cxt->hip;
    const int C = cxt->numChannels;
    const int staged = output && out_bytes + 16 <= DEC_KERNEL_COPY_LIMIT;

    if (staged)         /* output and state in ONE launch, no copy-engine command */
        arthip_copy2_by_kernel (hip->h_out, hip->d_out, (out_bytes + 3) & ~(size_t) 3, hip->h_state, hip->d_state, hip->state_bytes, hip->stream);
    else {
        if (output) arthip_d2h (output, hip->d_out, out_bytes, hip->stream);
        arthip_d2h (hip->h_state, hip->d_state, hip->state_bytes, hip->stream);
    }
    if (arthip_sync (hip->stream)) { fprintf (stderr, "artamd: decimator: %s\n", arthip_last_error ()); return 0; }
    if (staged) memcpy (output, hip->h_out, out_bytes);

    const unsigned char *m = hip->h_state;
    const unsigned long long total = *(const unsigned long long *) m;
    memcpy (cxt->feedback, m + ((unsigned char *) hip->d_feedback - hip->d_state), sizeof (art_s) * C);
    if (cxt->tpdf_generators) memcpy (cxt->tpdf_generators, m + ((unsigned char *) hip->d_gens - hip->d_state), sizeof (uint32_t) * C);
    if (cxt->noise_shapers) memcpy (cxt->noise_shapers, m + ((unsigned char *) hip->d_shapers - hip->d_state), sizeof (Biquad) * C);

    int delta = (int)(total - hip->clipped_seen);
    hip->clipped_seen = total;
    return delta;
}

/* a sharded context after a host-pointer call: every shard's state block comes back on the shard's own stream; clip counts add
 * up, the host mirrors are assembled channel slice by channel slice */
static int dec_finish_shards (Decimate *cxt)
{
    struct artamd_decimator *hip = cxt->hip;
    const int prev = arthip_current_device ();
    int clipped = 0;
    for (int k = 0; k < hip->nshards; ++k) {
        struct artamd_decimator *sp = hip->shards [k]->hip;
        arthip_set_device (sp->device);
        arthip_d2h (sp->h_state, sp->d_state, sp->state_bytes, sp->stream);
    }
    for (int k = 0; k < hip->nshards; ++k) {
        Decimate *leaf = hip->shards [k];
        struct artamd_decimator *sp = leaf->hip;
        const int first = hip->shard_first [k], width = hip->shard_first [k + 1] - first;
        arthip_set_device (sp->device);
        if (arthip_sync (sp->stream)) { pcm_fail ("sharded decimator: a shard's stream failed (its channels are not to be trusted)"); continue; }
        const unsigned char *m = sp->h_state;
        const unsigned long long total = *(const unsigned long long *) m;
        memcpy (cxt->feedback + first, m + ((unsigned char *) sp->d_feedback - sp->d_state), sizeof (art_s) * width);
        if (cxt->tpdf_generators) memcpy (cxt->tpdf_generators + first, m + ((unsigned char *) sp->d_gens - sp->d_state), sizeof (uint32_t) * width);
        if (cxt->noise_shapers) memcpy (cxt->noise_shapers + first, m + ((unsigned char *) sp->d_shapers - sp->d_state), sizeof (Biquad) * width);
        clipped += (int)(total - sp->clipped_seen);
        sp->clipped_seen = total;
    }
    if (prev >= 0) arthip_set_device (prev);
    return clipped;
}

int decimateProcessInterleavedLE (Decimate *cxt, const artsample_t *input, int numInputFrames, unsigned char *output)
{
    struct artamd_decimator *hip = cxt->hip;
    if (numInputFrames <= 0) return 0;
    const size_t samples = (size_t) numInputFrames * cxt->numChannels, in_bytes = samples * sizeof (art_s);
    ArtDecArgs a;
    ENTER_DEVICE (hip);

    if (dec_reserve (cxt, in_bytes, samples * cxt->outputBytes)) {
        fprintf (stderr, "artamd: decimator device allocation failed: %s\n", arthip_last_error ());
        LEAVE_DEVICE (hip);
        return 0;
    }
    if (in_bytes + 16 <= DEC_KERNEL_COPY_LIMIT) {
        memcpy (hip->h_in, input, in_bytes);
        arthip_copy_by_kernel (hip->d_in, hip->h_in, in_bytes, hip->stream);
    }
    else arthip_h2d (hip->d_in, input, in_bytes, hip->stream);
    int clipped;
    if (hip->nshards) {
        /* the whole interleaved buffer is staged on this context's device (one dense transfer each way), the shards work on it */
        const size_t out_bytes = samples * cxt->outputBytes;
        dec_sharded_call (cxt, hip->d_in, 0, numInputFrames, hip->d_out, 0);
        if (out_bytes + 16 <= DEC_KERNEL_COPY_LIMIT) {
            arthip_copy_by_kernel (hip->h_out, hip->d_out, (out_bytes + 3) & ~(size_t) 3, hip->stream);
            arthip_sync (hip->stream);
            memcpy (output, hip->h_out, out_bytes);
        }
        else { arthip_d2h (output, hip->d_out, out_bytes, hip->stream); arthip_sync (hip->stream); }
        clipped = dec_finish_shards (cxt);
    }
    else {
        dec_args (cxt, &a);
        dec_swap_if (cxt, arthip_decimate (&a, hip->d_in, numInputFrames, hip->d_out, hip->stream));
        clipped = dec_finish (cxt, output, samples * cxt->outputBytes);
    }
    LEAVE_DEVICE (hip);
    return clipped;
}

/* planar call of an ordinary context, enqueued only (dec_finish / dec_finish_shards waits) */
static int dec_planar_begin (Decimate *cxt, const artsample_t *const *input, int numInputFrames, unsigned char *const *output)
{
    struct artamd_decimator *hip = cxt->hip;
    const int C = cxt->numChannels;
    const size_t n = (size_t) numInputFrames, plane_bytes = n * cxt->outputBytes;
    ArtDecArgs a;

    if (dec_reserve (cxt, n * C * sizeof (art_s), plane_bytes * C)) {
        fprintf (stderr, "artamd: decimator device allocation failed: %s\n", arthip_last_error ());
        return -1;
    }
    dec_args (cxt, &a);
    for (int c = 0; c < C; ++c)
        arthip_h2d (hip->d_in + n * c, input [c], n * sizeof (art_s), hip->stream);
    arthip_decimate_planar (&a, hip->d_in, (long) n, numInputFrames, hip->d_out, (long) plane_bytes, hip->stream);
    for (int c = 0; c < C; ++c)
        arthip_d2h (output [c], hip->d_out + plane_bytes * c, plane_bytes, hip->stream);
    return 0;
}

int decimateProcessLE (Decimate *cxt, const artsample_t *const *input, int numInputFrames, unsigned char *const *output)
{
    struct artamd_decimator *hip = cxt->hip;
    if (numInputFrames <= 0) return 0;
    if (hip->nshards) {
        /* planes need no slicing: a shard's channels are a run of the caller's planes; all shards are enqueued before any is waited for */
        const int prev = arthip_current_device ();
        arthip_set_device (hip->device);                /* (the context's stream on the context's device) */
        arthip_sync (hip->stream);
        for (int k = 0; k < hip->nshards; ++k) {
            arthip_set_device (hip->shards [k]->hip->device);
            if (dec_planar_begin (hip->shards [k], input + hip->shard_first [k], numInputFrames, output + hip->shard_first [k])) {
                /* (counted; the shard's planes are the caller's host memory: silence instead of whatever was there) */
                pcm_fail ("sharded decimator: device allocation failed (a shard's planes zeroed)");
                for (int c = hip->shard_first [k]; c < hip->shard_first [k + 1]; ++c) memset (output [c], 0, (size_t) numInputFrames * cxt->outputBytes);
            }
        }
        if (prev >= 0) arthip_set_device (prev);
        return dec_finish_shards (cxt);
    }
    ENTER_DEVICE (hip);
    const int clipped = dec_planar_begin (cxt, input, numInputFrames, output) ? 0 : dec_finish (cxt, NULL, 0);
    LEAVE_DEVICE (hip);
    return clipped;
}

/* ------------------------------------------------------------------------------------------
 * Integer -> float ingest
 * ---------------------------------------------------------------------------------------- */

static art_s ingest_gain (double gain, int bits)
{
    return bits <= 8 ? (art_s)(gain / 128.0) : bits <= 16 ? (art_s)(gain / 32768.0) : (art_s)(gain / 8388608.0);
}

void floatIntegersLEDevice (const unsigned char *d_input, double inputGain, int inputBits, int inputBytes, int inputStride,
                            artsample_t *d_output, int numSamples, void *stream)
{
    if (inputBits > 24) return;
    arthip_ingest (d_input, ingest_gain (inputGain, inputBits), inputBits, inputBytes, inputStride, d_output, numSamples, stream);
}

/* the samples an item's runs start before its first one: run k begins at sample k * ART_INGEST_RUN - head, i.e. at byte
 * addr - head * sizeof (art_s) + 16 k, on a 16-byte boundary whenever the output is aligned to its sample size (else 0: scalar stores) */
int artamd_ingest_head (const void *d_output)
{
    const size_t addr = (size_t) d_output;
    return addr % sizeof (art_s) ? 0 : (int)(addr % 16 / sizeof (art_s));
}

/* many buffers, one launch: the items the single call would not skip, in list order, with their first tasks */
int floatIntegersBatchLEDevice (const unsigned char *const *d_inputs, const double *inputGains, const int *inputBits,
                                const int *inputBytes, const int *inputStrides, artsample_t *const *d_outputs,
                                const int *numSamples, int n, void *hipStream)
{
    int live = 0;
    for (int i = 0; i < n; ++i) {
        if (numSamples [i] <= 0 || inputBits [i] > 24) continue;
        if (!d_inputs [i] || !d_outputs [i]) { fprintf (stderr, "artamd: ingest batch: a NULL buffer pointer\n"); return -1; }
        ++live;
    }
    if (!live) return 0;
    ArtIngestItem *items = malloc (sizeof (ArtIngestItem) * (size_t) live);
    if (!items) { pcm_fail ("ingest batch: out of host memory"); return -1; }
    long tasks = 0;
    for (int i = 0, j = 0; i < n; ++i) {
        if (numSamples [i] <= 0 || inputBits [i] > 24) continue;
        ArtIngestItem *it = &items [j++];
        it->in = d_inputs [i]; it->out = d_outputs [i];
        it->task0 = tasks;
        it->gain_factor = ingest_gain (inputGains [i], inputBits [i]);
        it->bits = inputBits [i]; it->bytes = inputBytes [i]; it->stride = inputStrides [i]; it->count = numSamples [i];
        it->head = artamd_ingest_head (d_outputs [i]);
        tasks += ((long) numSamples [i] + it->head + ART_INGEST_RUN - 1) / ART_INGEST_RUN;
    }
    const int rc = arthip_ingest_batch (items, live, tasks, hipStream);
    free (items);
    if (rc) { pcm_fail ("ingest batch: the table could not be uploaded or the launch failed"); return -1; }
    return 1;
}

/* host-pointer form: process-wide scratch (device + page-locked), small calls by copy kernels */
static struct { unsigned char *d_in, *h_in; art_s *d_out, *h_out; size_t in_cap, out_cap; int device; } ingest_scratch = { .device = -1 };
static pthread_mutex_t ingest_lock = PTHREAD_MUTEX_INITIALIZER;

void floatIntegersLE (unsigned char *input, double inputGain, int inputBits, int inputBytes, int inputStride, artsample_t *output, int numSamples)
{
    if (numSamples <= 0 || inputBits > 24) return;
    const size_t in_bytes = (size_t) numSamples * inputStride * inputBytes, out_bytes = sizeof (art_s) * (size_t) numSamples;
    /* the last sample's trailing stride bytes may not exist in the caller's buffer */
    const size_t valid = in_bytes - (size_t)(inputStride - 1) * inputBytes;

    pthread_mutex_lock (&ingest_lock);
    const int device = arthip_current_device ();
    if (ingest_scratch.device != device) {
        arthip_free (ingest_scratch.d_in); arthip_free (ingest_scratch.d_out); arthip_host_free (ingest_scratch.h_in); arthip_host_free (ingest_scratch.h_out);
        memset (&ingest_scratch, 0, sizeof (ingest_scratch));
        ingest_scratch.device = device;
    }
    if (in_bytes + 16 > ingest_scratch.in_cap) {
        arthip_free (ingest_scratch.d_in); arthip_host_free (ingest_scratch.h_in);
        ingest_scratch.in_cap = (in_bytes + 16) * 2;
        ingest_scratch.d_in = arthip_malloc (ingest_scratch.in_cap); ingest_scratch.h_in = arthip_host_alloc (ingest_scratch.in_cap);
    }
    if (out_bytes + 16 > ingest_scratch.out_cap) {
        arthip_free (ingest_scratch.d_out); arthip_host_free (ingest_scratch.h_out);
        ingest_scratch.out_cap = (out_bytes + 16) * 2;
        ingest_scratch.d_out = arthip_malloc (ingest_scratch.out_cap); ingest_scratch.h_out = arthip_host_alloc (ingest_scratch.out_cap);
    }
    if (arthip_device_count () < 1 || !ingest_scratch.d_in || !ingest_scratch.d_out || !ingest_scratch.h_in || !ingest_scratch.h_out) {
        /* no CPU evaluation path exists: say so (counted: artamdErrorCount) and hand back silence rather than uninitialised memory */
        pcm_fail ("floatIntegersLE needs a HIP device and scratch memory (no CPU path; output zeroed)");
        memset (output, 0, out_bytes);
        ingest_scratch.in_cap = ingest_scratch.out_cap = 0;
        pthread_mutex_unlock (&ingest_lock);
        return;
    }
    const int small = in_bytes + out_bytes <= ((size_t) 1 << 20);
    if (small) {
        memcpy (ingest_scratch.h_in, input, valid);
        arthip_copy_by_kernel (ingest_scratch.d_in, ingest_scratch.h_in, (valid + 3) & ~(size_t) 3, NULL);
    }
    else arthip_h2d (ingest_scratch.d_in, input, valid, NULL);
    floatIntegersLEDevice (ingest_scratch.d_in, inputGain, inputBits, inputBytes, inputStride, ingest_scratch.d_out, numSamples, NULL);
    if (small) arthip_copy_by_kernel (ingest_scratch.h_out, ingest_scratch.d_out, out_bytes, NULL);
    else arthip_d2h (output, ingest_scratch.d_out, out_bytes, NULL);
    if (arthip_sync (NULL)) { pcm_fail ("floatIntegersLE kernel failed (output zeroed)"); memset (output, 0, out_bytes); }
    else if (small) memcpy (output, ingest_scratch.h_out, out_bytes);
    pthread_mutex_unlock (&ingest_lock);
}
