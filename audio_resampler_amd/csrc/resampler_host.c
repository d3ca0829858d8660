/* resampler_host.c — host (C) side of the MI355X sinc resampler.
 *
 * What runs here, on the CPU, is only what is inherently scalar and O(1)..O(log n) per call:
 *   - filter-bank design in fp64 (once per context)           reference resampler.c:1090-1133, :149-168
 *   - fixed-ratio resolution (gcd / auto low-pass)            reference resampler.c:310-356
 *   - the position state machine, replayed in CLOSED FORM     reference resampler.c:487-537 (loop form)
 *   - getters / dry runs                                       reference resampler.c:365-397, :853-968
 * Every output sample is computed on the GPU (sinc_fir.hip).  There is no CPU evaluation path:
 * without a device the init functions fail loudly.
 */
#define _USE_MATH_DEFINES
#define _POSIX_C_SOURCE 200809L
#include <limits.h>
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "art_internal.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

#define HIST_FRAMES(T) ((T) + (T) / 2)      /* frames of history kept in HBM between calls */

/* host-pointer calls up to this many bytes (in + out) go through page-locked staging buffers — the input by a copy kernel, the
 * output written there by the FIR kernels themselves, no copy-engine command at all —; larger ones are copied straight
 * from / to the caller's memory */
#define KERNEL_COPY_LIMIT ((size_t) 1 << 20)     /* staged transfers up to this size are made by a copy kernel, not a copy-engine command */
#define DIRECT_OUT_LIMIT ((size_t) 1 << 20)      /* staged outputs up to this size are written by the FIR kernels straight into the page-locked buffer */
#define STAGE_LIMIT ((size_t) 3 << 19)          /* 1.5 MB: measured on MI355X hosts, 8 ch x 988 taps: 16,384-frame calls 107 -> 92 us staged, 65,536-frame
                                                 * calls 176 us direct vs 235-378 staged (the CPU's own copies into and out of the staging cost more than
                                                 * the runtime's pipelined pageable path saves).  Environment ARTAMD_STAGE_LIMIT=bytes overrides (tests) */

struct BankEntry;
struct shard_pool;
struct artamd_resampler {
    int device;                             /* HIP device this context lives on (made current around every call) */
    void *stream;
    int own_stream;                         /* the stream was created by the library (shards of a sharded context) */
    /* a sharded context (RESAMPLE_MULTITHREADED with several devices / ARTAMD_SHARDS): no device state of its own, its
     * channels are spread over `nshards` ordinary contexts that run side by side (reference resampler.c:442-470 fans the
     * channels of ONE context out to worker threads; here to devices) */
    int nshards;
    Resample **shards;
    int *shard_first;                       /* first channel of each shard (nshards + 1 entries) */
    void *ev_parent, **ev_shard;            /* ordering events of the device-pointer calls */
    struct shard_pool *pool;                /* one worker thread per shard: the shards' launch sequences are enqueued side by side (NULL: by the caller, one after the other) */
    art_s *h_in, *h_out; size_t h_in_cap, h_out_cap;     /* page-locked staging of the host-pointer calls */
    struct BankEntry *bank;                 /* shared filter bank (bank_acquire / bank_release) */
    art_s *d_bank;                          /* = bank->dev */
    art_s *d_hist [2];                      /* ping-pong history, HIST x C interleaved */
    int cur;
    art_s *d_in;  size_t in_cap;            /* staging for host-pointer calls (bytes) */
    art_s *d_out; size_t out_cap;
    art_s *d_tmp; size_t tmp_cap;           /* planar <-> interleaved scratch */
    ArtamdSegment *segs; int seg_cap;
    int floor_active;                       /* ring index 0 is a hard history floor (after a flush-time rewind) */
    int kernel_pref, last_kernel;
    long long lin_origin;                    /* input frames appended since init / reset (ArtFirArgs.lin_origin) */
    unsigned int invariant_fallbacks;        /* launches the cut-invariant policy had to give to the general kernel (resampleHipCutInvariantFallbacks) */
    int stream_channels;                     /* a shard: channels of the whole stream (kernel choice); 0 otherwise */
    /* cached rational structure of the current ratio */
    double period_ratio; int period_out, period_in;
    /* optional HIP-event timing of FIR launches */
    int timing; void **ev; int ev_count, ev_cap; double prep_ms;
    art_s *d_patch; size_t patch_cap;        /* end-point extrapolation: samples computed on the host */
    void *d_scratch; size_t scratch_cap;     /* MFMA path: effective rows + canonical positions of one launch */
    void *d_pad; size_t pad_cap;             /* matrix path of a channel count the kernels are not compiled for: the groups' padded buffers (arthip_fir_pad_bytes) */
    void *d_planes; size_t planes_cap;       /* fixed-point matrix kernel: digit planes of one launch (flag word first) */
    int rows_off; void *d_rows; size_t rows_cap; void *rows_cache; void *last_masks;      /* ... its filter rows, kept across calls (art_internal.h), and where the last launch's row masks live */
    void *d_split; size_t split_cap;         /* K-split streaming kernel: arrival counters (zero at rest) + partial sums of one launch */
    int last_fixed [4];                      /* its last launch of the last call: flag value (0: none), mask words, chunks per tile, kernel form (art_hip.h) */
    unsigned int *d_fix; size_t fix_cap;    /* [0] per-launch, [1] running count of outputs the matrix kernels evaluated off-pattern */
    void *d_batch; size_t batch_cap;         /* argument table of the batched calls led by this context */
    void *d_group; size_t group_cap;         /* ... and of their grouped matrix-core launches (both tables are in flight in one batch call) */
    void *d_layout; size_t layout_cap;       /* ... and of the two transposing launches round the staged calls of a planar batch (resampleProcessBatchPlanarDevice) */
    art_s *d_tails; size_t tails_cap;        /* ... and the flush tails of every extrapolating context of such a call (resampleProcessAndFlushBatchInterleavedDevice) */
    void *d_sched; size_t sched_cap;         /* block and segment tables of the scheduled runs (resampleProcessScheduleInterleavedDevice) */
    void *d_sched_batch; size_t sched_batch_cap;     /* item, block and segment table of the many-stream schedules led by this context */
    unsigned long batch_stamp;               /* last batched call this context took part in (duplicate check) */
    int last_gathered;                       /* the last call or block ran in a launch shared by the batch or schedule entry (resampleHipLastGathered) */
};

static struct shard_pool *shard_pool_create (Resample *cxt, int n);
static void shard_pool_destroy (struct shard_pool *pool);


/* ------------------------------------------------------------------------------------------
 * Filter bank
 * ---------------------------------------------------------------------------------------- */

/* One polyphase row: windowed sinc centred (T/2 - 1 + phase) taps in, DC-normalised, rounded to
 * float from the centre outwards with the rounding error carried along. */
static void design_row (art_s *row, double *work, int T, double phase, double lowpass, int use_bh)
{
    const int mid = T / 2;
    double dc = 0.0;

    for (int k = 0; k < T; ++k) {
        double radians = fabs ((mid - 1) + phase - k) * M_PI;
        double wphase = radians / mid;
        double tap = 1.0;

        if (radians != 0.0) {
            tap = sin (radians * lowpass) / (radians * lowpass);
            tap *= use_bh ? 0.35875 + 0.48829 * cos (wphase) + 0.14128 * cos (2 * wphase) + 0.01168 * cos (3 * wphase)
                          : 0.5 * (1.0 + cos (wphase));
        }

        dc += work [k] = tap;
    }

    const double unity = 1.0 / dc;
    double residue = 0.0;

    /* visiting order mid, mid-1, mid+1, mid-2, ..., 0 */
    for (int step = 0, k = mid; step < T; ++step, k = (k >= mid) ? T - k - 1 : T - k) {
        work [k] *= unity;
        row [k] = (art_s)(work [k] - residue);
        residue += row [k] - work [k];
    }
}

void artamdBuildFilterBank (int T, int F, double lowpass, int flags, artsample_t *bank)
{
    double *work = malloc (sizeof (double) * (size_t) T);

    memset (bank, 0, sizeof (art_s) * (size_t)(F + 1) * T);

    for (int f = 0; f < F; ++f)
        design_row (bank + (size_t) f * T, work, T, (double) f / F, lowpass, flags & BLACKMAN_HARRIS);

    for (int k = 0; k < T; ++k)                         /* row F: row 0 one tap later */
        bank [(size_t) F * T + (k + 1) % T] = bank [k];

    bank [T - 1] = 0.0f;                                /* clear the two window outliers */
    bank [(size_t) F * T] = 0.0f;
    free (work);
}

/* ------------------------------------------------------------------------------------------
 * Position state machine in closed form
 *
 * The reference alternates "consume one input frame" / "emit one output frame" in a scalar loop
 * (resampler.c:494-529).  Output j (counted from the start of the call) sits at ring position
 * base + j/ratio and can be emitted once inputIndex > position + T/2.  Because fl(base + fl(j/ratio))
 * is monotone in j, the number of outputs reachable with a given inputIndex is found by bisection,
 * and the ring rewinds (every 15T consumed frames) split the call into segments with their own
 * `base`.  The arithmetic that decides emit-vs-consume is the reference's own comparison, so the
 * counts and the carried position are bit-identical to the loop.
 * ---------------------------------------------------------------------------------------- */

static int plan_call (ArtamdPosition *p, int nIn, int cap, double ratio, ResampleResult *result,
                      ArtamdSegment *segs, int max_segs, int *lin_floor_out, int keep_offset);

int artamdPlanCall (ArtamdPosition *p, int nIn, int cap, double ratio, ResampleResult *result,
                    ArtamdSegment *segs, int max_segs, int *lin_floor_out)
{
    return plan_call (p, nIn, cap, ratio, result, segs, max_segs, lin_floor_out, 0);
}

/* keep_offset: the call is the silent first part of a caller's call that the library split in two (consume_silently): the
 * end-of-call re-quantisation of the position (resampler.c:533-535) belongs to the second part only */
static int plan_call (ArtamdPosition *p, int nIn, int cap, double ratio, ResampleResult *result,
                      ArtamdSegment *segs, int max_segs, int *lin_floor_out, int keep_offset)
{
    const int T = p->numTaps, half = T / 2, ring = 16 * T, drop = 15 * T;
    double base = p->outputOffset;
    int wp = p->inputIndex, flags = p->flags;
    int nseg = 0;

    if (flags & RESAMPLE_FIXED_RATIO) ratio = p->fixedRatio;
    if (flags & RESAMPLER_FLUSHED) nIn = 0;

    int lin_base = HIST_FRAMES (T) - wp;
    int lin_floor = p->floorActive ? lin_base : INT_MIN;

    if (nIn < 0) {                                      /* flush: half a window of silence is appended */
        if (ring - wp < half) {                         /* resampler.c:667-672; see DESIGN.md "reference bugs" */
            base -= drop; wp -= drop; lin_base += drop;
            p->floorActive = 1;
            lin_floor = lin_base;
        }
        flags |= RESAMPLER_FLUSHED;
        wp += half;
        nIn = 0;
    }

    unsigned int made = 0, used = 0;
    const unsigned int ucap = cap > 0 ? (unsigned int) cap : 0;
    long left = nIn;

#define PUSH_SEGMENT() do { if (nseg < max_segs) { segs [nseg].first_output = made; segs [nseg].lin_base = lin_base; \
                                                   segs [nseg].base_offset = base; } nseg++; } while (0)
    PUSH_SEGMENT ();

    if (!(ratio > 0.0))                                 /* the reference never terminates sensibly here */
        cap = 0;

    while (made < ucap && cap > 0) {
        long reach = (long) wp + left;
        int top = reach < ring ? (int) reach : ring;    /* highest inputIndex reachable in this ring epoch */
        double limit = (double)(top - half);
        unsigned int lo = made, hi = ucap;

        /* two bisection steps placed AT the arithmetic estimate (any probe inside [lo, hi) is a valid step of the same
         * monotone search, so the answer is unchanged): the answer is the estimate rounded up unless the roundings of the
         * reference's own expression disagree with it by one, so the two probes e, e + 1 normally close the interval — two
         * divisions per ring epoch instead of 21 (a 1M-frame call has 70-180 epochs with long filters, 1,456 at 48 taps, where
         * the planner, not the GPU, set the pace of a call) */
        {
            const double est = (limit - base) * ratio;
            if (est > 2.0 && est < 4.0e9) {
                const unsigned int e = (unsigned int) est;
                for (int probe = 0; probe < 2; ++probe) {
                    const unsigned int mid = probe ? e + 1 : e;
                    if (mid >= lo && mid < hi) { if (base + (double) mid / ratio < limit) lo = mid + 1; else hi = mid; }
                }
            }
        }

        while (lo < hi) {                               /* first j with position(j) >= limit */
            unsigned int mid = lo + (hi - lo) / 2;
            if (base + (double) mid / ratio < limit) lo = mid + 1; else hi = mid;
        }

        if (lo > made) {                                /* inputs consumed on the way to output lo-1 */
            long need = (long) floor (base + (double)(lo - 1) / ratio) + half + 1;
            if (need > wp) { used += (unsigned int)(need - wp); left -= need - wp; wp = (int) need; }
            made = lo;
        }

        if (made == ucap) break;

        used += (unsigned int)(top - wp); left -= top - wp; wp = top;

        if (left <= 0) break;                           /* output `made` needs input we do not have */

        base -= drop; wp -= drop; lin_base += drop;     /* ring full: rewind, then take the frame that forced it */
        wp++; used++; left--;
        PUSH_SEGMENT ();
    }
#undef PUSH_SEGMENT

    base += made ? (double) made / ratio : 0.0;

    if ((flags & RESAMPLER_SNAP_OFFSET) && !keep_offset)
        base = floor (base) + floor ((base - floor (base)) * p->numFilters + 0.5) / p->numFilters;

    p->outputOffset = base; p->inputIndex = wp; p->flags = flags;
    result->input_used = used; result->output_generated = made;
    if (lin_floor_out) *lin_floor_out = lin_floor;
    return nseg;
}

/* smallest p/q (q <= 4096) whose double quotient equals `ratio` bit for bit; 0 if none */
static void find_period (double ratio, int *p_out, int *q_out)
{
    *p_out = *q_out = 0;
    if (!(ratio > 1.0 / 4096 && ratio < 4096)) return;

    double x = ratio;
    long h0 = 0, h1 = 1, k0 = 1, k1 = 0;               /* continued-fraction convergents h/k */

    for (int it = 0; it < 32; ++it) {
        double a = floor (x);
        long h2 = (long) a * h1 + h0, k2 = (long) a * k1 + k0;
        if (k2 > 4096 || h2 > 4096 * 4096L) return;
        if ((double) h2 / (double) k2 == ratio) { if (h2 <= 4096) { *p_out = (int) h2; *q_out = (int) k2; } return; }
        h0 = h1; h1 = h2; k0 = k1; k1 = k2;
        double frac = x - a;
        if (frac < 1e-12) return;
        x = 1.0 / frac;
    }
}

/* ------------------------------------------------------------------------------------------
 * Contexts
 * ---------------------------------------------------------------------------------------- */

static void *grow_pinned (void *host, size_t *cap, size_t need)
{
    if (need <= *cap) return host;
    arthip_host_free (host);
    size_t want = need + need / 2 + 4096;
    host = arthip_host_alloc (want);
    *cap = host ? want : 0;
    return host;
}

/* ------------------------------------------------------------------------------------------
 * Devices.  An ordinary context lives on the HIP device that is current when it is created and makes that device current
 * around every call it serves, whatever the calling thread had selected.  A context created with RESAMPLE_MULTITHREADED
 * spreads its channels over the devices of this list (artamdSetDevices, or environment ARTAMD_DEVICES="0,1,2,3"; default:
 * every visible device) — the reference's one-worker-per-channel fan-out (resampler.c:185-186, :442-470) with GPUs for
 * threads.  ARTAMD_SHARDS=n forces the number of shards (several shards per device, or sharding on a single device: the
 * way the path is tested on a one-GPU box).
 * ---------------------------------------------------------------------------------------- */
#define MAX_DEVICES ART_MAX_DEVICES
static int dev_list [MAX_DEVICES], dev_count = -1;        /* -1: not resolved yet */
static pthread_mutex_t dev_lock = PTHREAD_MUTEX_INITIALIZER;

static void resolve_devices (void)
{
    const int visible = arthip_device_count ();
    const char *env = getenv ("ARTAMD_DEVICES");

    dev_count = 0;
    if (env && *env) {
        while (*env && dev_count < MAX_DEVICES) {
            char *end;
            long d = strtol (env, &end, 10);
            if (end == env) break;
            if (d >= 0 && d < visible) dev_list [dev_count++] = (int) d;
            else fprintf (stderr, "artamd: ARTAMD_DEVICES names device %ld, %d visible: ignored\n", d, visible);
            env = (*end == ',') ? end + 1 : end;
        }
    }
    if (!dev_count)
        for (int d = 0; d < visible && d < MAX_DEVICES; ++d) dev_list [dev_count++] = d;
}

int artamdSetDevices (const int *devices, int count)
{
    const int visible = arthip_device_count ();
    int rc = 0;

    pthread_mutex_lock (&dev_lock);
    if (count <= 0 || !devices) resolve_devices ();
    else {
        for (int i = 0; i < count; ++i)
            if (devices [i] < 0 || devices [i] >= visible) rc = -1;
        if (!rc) {
            dev_count = count < MAX_DEVICES ? count : MAX_DEVICES;
            for (int i = 0; i < dev_count; ++i) dev_list [i] = devices [i];
        }
    }
    pthread_mutex_unlock (&dev_lock);
    return rc;
}

/* how many shards a MULTITHREADED context of `channels` channels gets (0 or 1: an ordinary context) and on which device
 * shard s lives.  Left to itself a context spreads over the listed devices with at least two channels per shard (a stereo
 * stream is not worth two devices' launches: ARTAMD_MIN_SHARD_CHANNELS); ARTAMD_SHARDS forces the count.  The slice kernels
 * of a shard read and write the caller's buffers on `home` in place: a device with no peer route to `home` (IOMMU,
 * containers, mixed topology — a page fault, not an error code, if it were used) is replaced by `home` itself. */
int artamd_batch_distinct (const void *const *items, int n, unsigned long *(*stamp_of) (const void *item), const char *what, const char *noun)
{
    static unsigned long calls;
    const unsigned long stamp = __atomic_add_fetch (&calls, 1, __ATOMIC_RELAXED);
    for (int i = 0; i < n; ++i) {
        if (!items [i]) { fprintf (stderr, "artamd: %s batch: a NULL %s\n", what, noun); return -1; }
        unsigned long *seen = stamp_of (items [i]);
        if (*seen == stamp) { fprintf (stderr, "artamd: %s batch: a %s appears twice\n", what, noun); return -1; }
        *seen = stamp;
    }
    return 0;
}

int artamd_shard_plan (int channels, int home, int *devices_out)
{
    pthread_mutex_lock (&dev_lock);
    if (dev_count < 0) resolve_devices ();
    int n = dev_count > 1 ? dev_count : 0;
    const char *env = getenv ("ARTAMD_SHARDS"), *min_env = getenv ("ARTAMD_MIN_SHARD_CHANNELS");
    if (env && *env) n = atoi (env);
    else {
        const int per = min_env && *min_env && atoi (min_env) > 0 ? atoi (min_env) : 2;
        if (n > channels / per) n = channels / per;
    }
    if (n > channels) n = channels;
    if (n > MAX_DEVICES) n = MAX_DEVICES;
    for (int s = 0; s < n; ++s) devices_out [s] = dev_count ? dev_list [s % dev_count] : 0;
    pthread_mutex_unlock (&dev_lock);
    if (home >= 0)
        for (int s = 0; s < n; ++s)
            if (devices_out [s] != home && !arthip_enable_peer (devices_out [s], home)) {
                static int warned;
                if (!warned++) fprintf (stderr, "artamd: device %d cannot address device %d's memory (no peer access): its shards stay on device %d\n", devices_out [s], home, home);
                devices_out [s] = home;
            }
    return n;
}

/* ------------------------------------------------------------------------------------------
 * Filter banks are shared: a service opens thousands of contexts with a handful of presets, a bank is up to 4 MB of HBM
 * and milliseconds of double-precision design work.  Contexts with the same (taps, filters, low-pass ratio, window) on the
 * same device reference ONE device bank (read-only to every kernel) and copy the designed rows for their own host table
 * (`filters` stays a private, writable array as in the reference).  Freed with its last context.
 * ---------------------------------------------------------------------------------------- */
typedef struct BankEntry {
    int T, F, bh, device, refs;
    double lowpass;
    art_s *host, *dev;
    struct BankEntry *next;
} BankEntry;

static BankEntry *bank_list;
static pthread_mutex_t bank_lock = PTHREAD_MUTEX_INITIALIZER;

static BankEntry *bank_acquire (int T, int F, double lowpass, int flags)
{
    const int bh = (flags & BLACKMAN_HARRIS) != 0, device = arthip_current_device ();
    const size_t bytes = sizeof (art_s) * (size_t)(F + 1) * T;
    BankEntry *e;

    pthread_mutex_lock (&bank_lock);
    for (e = bank_list; e; e = e->next)
        if (e->T == T && e->F == F && e->bh == bh && e->device == device && e->lowpass == lowpass) { e->refs++; break; }
    if (!e && (e = calloc (1, sizeof (*e)))) {
        e->T = T; e->F = F; e->bh = bh; e->device = device; e->lowpass = lowpass; e->refs = 1;
        e->host = malloc (bytes);
        e->dev = arthip_malloc (bytes);
        if (e->host) artamdBuildFilterBank (T, F, lowpass, flags, e->host);
        if (!e->host || !e->dev || arthip_h2d (e->dev, e->host, bytes, NULL) || arthip_sync (NULL)) {
            arthip_free (e->dev); free (e->host); free (e); e = NULL;
        }
        else { e->next = bank_list; bank_list = e; }
    }
    pthread_mutex_unlock (&bank_lock);
    return e;
}

static void bank_release (BankEntry *e)
{
    if (!e) return;
    pthread_mutex_lock (&bank_lock);
    if (--e->refs == 0) {
        for (BankEntry **p = &bank_list; *p; p = &(*p)->next)
            if (*p == e) { *p = e->next; break; }
        arthip_free (e->dev); free (e->host); free (e);
    }
    pthread_mutex_unlock (&bank_lock);
}

/* an ordinary context on the current device (parameters already validated, lowpassRatio normalised) */
static Resample *init_leaf (int numChannels, int numTaps, int numFilters, double lowpassRatio, int flags, int private_stream)
{
    Resample *cxt = calloc (1, sizeof (Resample));
    struct artamd_resampler *hip = calloc (1, sizeof (*hip));
    const size_t bank_count = (size_t)(numFilters + 1) * numTaps;
    const size_t hist_bytes = sizeof (art_s) * (size_t) HIST_FRAMES (numTaps) * numChannels;

    if (!cxt || !hip) {
        fprintf (stderr, "artamd: out of memory\n");
        free (cxt); free (hip);
        return NULL;
    }

    cxt->hip = hip;
    cxt->numChannels = numChannels;
    cxt->numSamples = numTaps * 16;
    cxt->numFilters = numFilters;
    cxt->numTaps = numTaps;
    cxt->flags = flags;
    cxt->lowpassRatio = lowpassRatio;
    cxt->outputOffset = numTaps / 2;
    cxt->inputIndex = numTaps;
    hip->device = arthip_current_device ();
    // (A/B runs and the PCM-level tests of programs that cannot call resampleHipSetKernel — the reference's own art / artest binaries:
    // ARTAMD_KERNEL=<n> is the kernel preference every new context starts with, see include/art_hip.h; anything but a documented
    // preference is ignored, with one warning per process)
    {
        const char *env = getenv ("ARTAMD_KERNEL");
        if (env && *env) {
            char *end;
            const long k = strtol (env, &end, 10);
            if (!*end && (k == 0 || k == 1 || k == 2 || (k >= 5 && k <= 9))) hip->kernel_pref = (int) k;
            else { static int warned; if (!warned++) fprintf (stderr, "artamd: ARTAMD_KERNEL=%s is not a kernel preference (0, 1, 2, 5-9): ignored\n", env); }
        }
    }
    if (private_stream) { hip->stream = arthip_stream_create (); hip->own_stream = hip->stream != NULL; }

    /* the bank: shared on the device, a private host copy exposed through the reference's `filters` row-pointer table */
    hip->bank = bank_acquire (numTaps, numFilters, lowpassRatio, flags);
    art_s *bank = malloc (sizeof (art_s) * bank_count);
    cxt->filters = malloc (sizeof (art_s *) * (size_t)(numFilters + 1));
    if (!hip->bank || !bank || !cxt->filters) {
        fprintf (stderr, "artamd: filter bank allocation failed: %s\n", arthip_last_error ());
        free (bank); free (cxt->filters); cxt->filters = NULL;
        resampleFree (cxt);
        return NULL;
    }
    memcpy (bank, hip->bank->host, sizeof (art_s) * bank_count);
    for (int f = 0; f <= numFilters; ++f)
        cxt->filters [f] = bank + (size_t) f * numTaps;

    hip->d_bank = hip->bank->dev;
    hip->d_hist [0] = arthip_malloc (hist_bytes);
    hip->d_hist [1] = arthip_malloc (hist_bytes);
    hip->seg_cap = 64;
    hip->segs = malloc (sizeof (ArtamdSegment) * hip->seg_cap);

    if (!hip->d_hist [0] || !hip->d_hist [1] || !hip->segs || (private_stream && !hip->stream) ||
        arthip_zero (hip->d_hist [0], hist_bytes, hip->stream) || arthip_zero (hip->d_hist [1], hist_bytes, hip->stream) ||
        arthip_sync (hip->stream)) {
        fprintf (stderr, "artamd: device allocation failed: %s\n", arthip_last_error ());
        resampleFree (cxt);
        return NULL;
    }

    if (flags & EXTRAPOLATE_ENDPOINTS)
        cxt->flags |= EXTRAPOLATE_PREFILL;

    return cxt;
}

/* a sharded context: `count` ordinary contexts on devices [s], each with a contiguous channel slice and its own stream */
static Resample *init_sharded (int numChannels, int numTaps, int numFilters, double lowpassRatio, int flags, int count, const int *devices)
{
    Resample *cxt = calloc (1, sizeof (Resample));
    struct artamd_resampler *hip = calloc (1, sizeof (*hip));
    const int prev = arthip_current_device ();

    if (!cxt || !hip) { free (cxt); free (hip); return NULL; }
    cxt->hip = hip;
    cxt->numChannels = numChannels;
    cxt->numSamples = numTaps * 16;
    cxt->numFilters = numFilters;
    cxt->numTaps = numTaps;
    cxt->flags = flags;
    cxt->lowpassRatio = lowpassRatio;
    cxt->outputOffset = numTaps / 2;
    cxt->inputIndex = numTaps;
    hip->device = prev;                                  /* device-pointer calls: where the caller's buffers are expected */
    hip->shards = calloc ((size_t) count, sizeof (Resample *));
    hip->shard_first = calloc ((size_t) count + 1, sizeof (int));
    hip->ev_shard = calloc ((size_t) count, sizeof (void *));
    hip->ev_parent = arthip_order_event_create ();
    int ok = hip->shards && hip->shard_first && hip->ev_shard && hip->ev_parent;

    /* Contiguous channel slices.  A shard decides its kernels as its whole stream would (stream_channels), and the matrix-core
     * kernels are compiled for 1, 2, 4, 8, 16 and 32 channels: with every slice one of those widths all shards of a stream run the
     * same kernels — the ordinary context's bits.  So the channels are written as a sum of `count` such widths where that is possible
     * (binary digits of the channel count, the largest part halved until there are enough: 12 over 5 = 4 2 2 2 2, 8 over 3 = 4 2 2);
     * where it is not (7 channels on 2 devices) the slices are balanced.  A slice — or a stream — of any other width runs its matrix-path
     * launches in groups of a compiled width (fir_dispatch.hip, fir_in_groups): a channel's arithmetic depends neither on its group's
     * width nor on its neighbours, so channels of one stream never get different arithmetic whatever the slices are. */
    int widths [MAX_DEVICES], parts = 0;
    {
        int left = numChannels;
        while (left > 0 && parts < count) {              /* the channel count's binary digits, 32 at most per part */
            int w = 32;
            while (w > left) w >>= 1;
            widths [parts++] = w; left -= w;
        }
        if (left) parts = 0;                             /* (more parts than shards) */
    }
    while (parts && parts < count) {                     /* halve the largest part until every shard has one */
        int big = 0;
        for (int i = 1; i < parts; ++i) if (widths [i] >= widths [big]) big = i;      /* (the last of the widest: wide slices first) */
        if (widths [big] == 1) break;
        widths [big] >>= 1;
        for (int i = parts; i > big + 1; --i) widths [i] = widths [i - 1];
        widths [big + 1] = widths [big];
        ++parts;
    }
    if (parts != count) {
        const int base = numChannels / count, extra = numChannels % count;
        for (int s = 0; s < count; ++s) widths [s] = base + (s < extra ? 1 : 0);
    }
    for (int s = 0; ok && s < count; ++s) {
        const int width = widths [s];
        hip->shard_first [s + 1] = hip->shard_first [s] + width;
        arthip_set_device (devices [s]);                  /* (artamd_shard_plan has made sure it can address `prev`'s memory) */
        hip->shards [s] = init_leaf (width, numTaps, numFilters, lowpassRatio, flags & ~RESAMPLE_MULTITHREADED, 1);
        hip->ev_shard [s] = arthip_order_event_create ();
        hip->nshards = s + 1;
        ok = hip->shards [s] && hip->ev_shard [s];
        if (ok) hip->shards [s]->hip->stream_channels = numChannels;
    }
    if (prev >= 0) arthip_set_device (prev);

    if (ok) {       /* `filters`: a private copy of the rows, as in every context */
        const size_t bank_count = (size_t)(numFilters + 1) * numTaps;
        art_s *bank = malloc (sizeof (art_s) * bank_count);
        cxt->filters = malloc (sizeof (art_s *) * (size_t)(numFilters + 1));
        if (bank && cxt->filters) {
            memcpy (bank, hip->shards [0]->filters [0], sizeof (art_s) * bank_count);
            for (int f = 0; f <= numFilters; ++f) cxt->filters [f] = bank + (size_t) f * numTaps;
        }
        else { free (bank); free (cxt->filters); cxt->filters = NULL; ok = 0; }
    }
    if (!ok) {
        fprintf (stderr, "artamd: sharded context: allocation failed: %s\n", arthip_last_error ());
        resampleFree (cxt);
        return NULL;
    }
    cxt->flags = hip->shards [0]->flags | RESAMPLE_MULTITHREADED;
    hip->pool = shard_pool_create (cxt, hip->nshards);       /* (NULL: the calling thread enqueues the shards one after the other) */
    return cxt;
}

Resample *resampleInit (int numChannels, int numTaps, int numFilters, double lowpassRatio, int flags)
{
    if (lowpassRatio > 0.0 && lowpassRatio < 1.0)
        flags |= INCLUDE_LOWPASS;
    else {
        flags &= ~INCLUDE_LOWPASS;
        lowpassRatio = 1.0;
    }

    if ((numTaps & 3) || numTaps <= 0 || numTaps > 1024) {
        fprintf (stderr, "must 4-1024 filter taps, and a multiple of 4!\n");
        return NULL;
    }

    if (numFilters < 1 || numFilters > 1024) {
        fprintf (stderr, "must be 1-1024 filters!\n");
        return NULL;
    }

    if (numChannels < 1) {
        fprintf (stderr, "must have at least one channel!\n");
        return NULL;
    }

    if (arthip_device_count () < 1) {
        fprintf (stderr, "artamd: no usable HIP device (this library has no CPU path): %s\n", arthip_last_error ());
        return NULL;
    }

    { const char *env = getenv ("ARTAMD_STRICT"); if (env && *env && *env != '0') flags |= RESAMPLE_STRICT_ORDER; }

    if ((flags & RESAMPLE_MULTITHREADED) && numChannels > 1) {
        int devices [MAX_DEVICES];
        const int count = artamd_shard_plan (numChannels, arthip_current_device (), devices);
        if (count > 1)
            return init_sharded (numChannels, numTaps, numFilters, lowpassRatio, flags, count, devices);
    }

    return init_leaf (numChannels, numTaps, numFilters, lowpassRatio, flags, 0);
}

static unsigned long gcd_of (unsigned long a, unsigned long b)
{
    while (b) { unsigned long r = a % b; a = b; b = r; }
    return a;
}

Resample *resampleFixedRatioInit (int numChannels, int numTaps, int maxFilters, double sourceRate, double destinRate, int lowpassFreq, int flags)
{
    double lowpass = lowpassFreq / (destinRate / 2.0);
    const double ratio = destinRate / sourceRate;

    if (lowpassFreq > destinRate / 2.0) {
        fprintf (stderr, "lowpass frequency must be lower than destination Nyquist!\n");
        return NULL;
    }

    /* integer rates whose reduced numerator fits the filter budget need no interpolation at all */
    if (sourceRate == floor (sourceRate) && destinRate == floor (destinRate) && !(flags & NO_FILTER_REDUCTION)) {
        unsigned long phases = (unsigned long) destinRate / gcd_of ((unsigned long) sourceRate, (unsigned long) destinRate);

        if (phases <= (unsigned long) maxFilters) {
            flags &= ~SUBSAMPLE_INTERPOLATE;
            maxFilters = (int) phases;

            if (maxFilters & (maxFilters - 1))          /* phases not a power of two: re-quantise per call */
                flags |= RESAMPLER_SNAP_OFFSET;
        }
    }

    if (!lowpassFreq && (flags & INCLUDE_LOWPASS) && destinRate < sourceRate) {
        lowpass = 1.0 - (7.5 / numTaps / ratio);
        if (lowpass < 0.8) lowpass = 0.8;
        if (lowpass < ratio) lowpass = ratio;
    }

    Resample *cxt = resampleInit (numChannels, numTaps, maxFilters, lowpass * ratio, flags | RESAMPLE_FIXED_RATIO);

    if (cxt) {
        cxt->fixedRatio = destinRate / sourceRate;
        for (int k = 0; k < cxt->hip->nshards; ++k)
            cxt->hip->shards [k]->fixedRatio = cxt->fixedRatio;
    }

    return cxt;
}

static int trace_on = -1;
static void trace_report (void);

void resampleFree (Resample *cxt)
{
    if (!cxt) return;
    trace_report ();                        /* (ARTAMD_HOST_TRACE: per-context figures) */

    struct artamd_resampler *hip = cxt->hip;

    if (hip) {
        shard_pool_destroy (hip->pool);
        for (int k = 0; k < hip->nshards; ++k) {
            resampleFree (hip->shards [k]);
            arthip_event_destroy (hip->ev_shard [k]);
        }
        ENTER_DEVICE (hip);
        if (!hip->shards) arthip_sync (hip->stream);
        arthip_event_destroy (hip->ev_parent);
        free (hip->shards); free (hip->shard_first); free (hip->ev_shard);
        bank_release (hip->bank); arthip_free (hip->d_hist [0]); arthip_free (hip->d_hist [1]);
        {   /* every device buffer the context may have grown (NULL where it never did) */
            void *const device_buffers [] = { hip->d_in, hip->d_out, hip->d_tmp, hip->d_fix, hip->d_scratch, hip->d_pad, hip->d_planes, hip->d_rows,
                                              hip->d_split, hip->d_patch, hip->d_batch, hip->d_group, hip->d_layout, hip->d_tails, hip->d_sched, hip->d_sched_batch };
            for (size_t i = 0; i < sizeof (device_buffers) / sizeof (device_buffers [0]); ++i) arthip_free (device_buffers [i]);
        }
        if (hip->rows_cache) { arthip_fir_rows_cache_free (hip->rows_cache); free (hip->rows_cache); }
        arthip_host_free (hip->h_in); arthip_host_free (hip->h_out);
        for (int i = 0; i < hip->ev_cap; ++i) arthip_event_destroy (hip->ev [i]);
        if (hip->own_stream) arthip_stream_destroy (hip->stream);
        LEAVE_DEVICE (hip);
        free (hip->ev);
        free (hip->segs);
        free (hip);
    }

    if (cxt->filters) { free (cxt->filters [0]); free (cxt->filters); }
    free (cxt);
}

/* the host part of resampleReset (the device part: both history buffers zero, in stream order before the next call) */
static void reset_host (Resample *cxt)
{
    struct artamd_resampler *hip = cxt->hip;
    hip->floor_active = 0; hip->lin_origin = 0;
    cxt->outputOffset = cxt->numTaps / 2;
    cxt->inputIndex = cxt->numTaps;

    if (cxt->flags & EXTRAPOLATE_ENDPOINTS)
        cxt->flags |= EXTRAPOLATE_PREFILL;

    cxt->flags &= ~RESAMPLER_FLUSHED;
}

void resampleReset (Resample *cxt)
{
    struct artamd_resampler *hip = cxt->hip;

    for (int k = 0; k < hip->nshards; ++k)
        resampleReset (hip->shards [k]);

    if (!hip->nshards) {
        const size_t hist_bytes = sizeof (art_s) * (size_t) HIST_FRAMES (cxt->numTaps) * cxt->numChannels;
        ENTER_DEVICE (hip);
        arthip_zero (hip->d_hist [0], hist_bytes, hip->stream);
        arthip_zero (hip->d_hist [1], hist_bytes, hip->stream);
        LEAVE_DEVICE (hip);
    }
    reset_host (cxt);
}

double resampleGetLowpassRatio (Resample *cxt) { return cxt->lowpassRatio; }
int resampleGetNumFilters (Resample *cxt) { return cxt->numFilters; }
int resampleInterpolationUsed (Resample *cxt) { return cxt->flags & SUBSAMPLE_INTERPOLATE; }

double resampleGetPosition (Resample *cxt)
{
    return cxt->outputOffset + (cxt->numTaps / 2.0) - cxt->inputIndex;
}

void resampleAdvancePosition (Resample *cxt, double delta)
{
    if (delta < 0.0)
        fprintf (stderr, "resampleAdvancePosition() can only advance forward!\n");
    else if (!(cxt->flags & SUBSAMPLE_INTERPOLATE) && floor (delta) != delta)
        fprintf (stderr, "resampleAdvancePosition() cannot advance partial samples without interpolation!\n");
    else {
        cxt->outputOffset += delta;
        for (int k = 0; k < cxt->hip->nshards; ++k)      /* the same addition on the same value: the shards stay in step */
            cxt->hip->shards [k]->outputOffset += delta;
    }
}

/* Dry runs.  These step the position by repeated addition of 1/ratio (reference resampler.c:874, :912)
 * — deliberately NOT the division form the real run uses — so they are replayed as loops. */
unsigned int resampleGetRequiredSamples (Resample *cxt, int numOutputFrames, double ratio)
{
    const int half = cxt->numTaps / 2, drop = cxt->numSamples - cxt->numTaps;
    int wp = cxt->inputIndex;
    double pos = cxt->outputOffset;
    unsigned int used = 0;

    if (cxt->flags & RESAMPLE_FIXED_RATIO) ratio = cxt->fixedRatio;
    if (!(ratio > 0.0)) return 0;

    while (numOutputFrames > 0)
        if (pos >= wp - half) {
            if (wp == cxt->numSamples) { pos -= drop; wp -= drop; }
            wp++; used++;
        }
        else { pos += 1.0 / ratio; numOutputFrames--; }

    return used;
}

unsigned int resampleGetExpectedOutput (Resample *cxt, int numInputFrames, double ratio)
{
    const int half = cxt->numTaps / 2, drop = cxt->numSamples - cxt->numTaps;
    int wp = cxt->inputIndex;
    double pos = cxt->outputOffset;
    unsigned int made = 0;

    if (cxt->flags & RESAMPLE_FIXED_RATIO) ratio = cxt->fixedRatio;
    if (!(ratio > 0.0)) return 0;

    if (cxt->flags & RESAMPLER_FLUSHED) numInputFrames = 0;
    else if (numInputFrames < 0) wp += half;

    for (;;)
        if (pos >= wp - half) {
            if (numInputFrames <= 0) break;
            if (wp == cxt->numSamples) { pos -= drop; wp -= drop; }
            wp++; numInputFrames--;
        }
        else { pos += 1.0 / ratio; made++; }

    return made;
}

/* ------------------------------------------------------------------------------------------
 * Processing
 * ---------------------------------------------------------------------------------------- */

/* Work already enqueued on the old stream (history ping-pong, matrix-path scratch, staging) must not race with what the
 * next call puts on the new one: the old stream is drained before the swap. */
void resampleHipSetStream (Resample *cxt, void *stream)
{
    struct artamd_resampler *hip = cxt->hip;
    if (hip->stream == stream) return;
    ENTER_DEVICE (hip);
    arthip_sync (hip->stream);          /* (a sharded context's own stream carries its staging copies and the shards' completion events) */
    if (hip->own_stream) { arthip_stream_destroy (hip->stream); hip->own_stream = 0; }
    hip->stream = stream;
    LEAVE_DEVICE (hip);
}

void resampleHipSynchronize (Resample *cxt)
{
    struct artamd_resampler *hip = cxt->hip;
    for (int k = 0; k < hip->nshards; ++k) resampleHipSynchronize (hip->shards [k]);
    ENTER_DEVICE (hip);
    arthip_sync (hip->stream);
    LEAVE_DEVICE (hip);
}

void resampleHipSetCutInvariant (Resample *cxt, int on)
{
    resampleHipSetKernel (cxt, on ? ART_KERNEL_INVARIANT : ART_KERNEL_AUTO);
}

unsigned int resampleHipCutInvariantFallbacks (Resample *cxt)
{
    unsigned int n = cxt->hip->invariant_fallbacks;
    for (int k = 0; k < cxt->hip->nshards; ++k) n += resampleHipCutInvariantFallbacks (cxt->hip->shards [k]);
    return n;
}

void resampleHipSetKernel (Resample *cxt, int which)
{
    cxt->hip->kernel_pref = which;
    for (int k = 0; k < cxt->hip->nshards; ++k) resampleHipSetKernel (cxt->hip->shards [k], which);
}

void resampleHipKeepRows (Resample *cxt, int on)
{
    cxt->hip->rows_off = !on;
    for (int k = 0; k < cxt->hip->nshards; ++k) resampleHipKeepRows (cxt->hip->shards [k], on);
}

int resampleHipGetDevice (Resample *cxt) { return cxt->hip->device; }
int resampleHipNumShards (Resample *cxt) { return cxt->hip->nshards; }
int resampleHipLastGathered (Resample *cxt) { return cxt->hip->last_gathered; }

int resampleHipShardInfo (Resample *cxt, int shard, int *device, int *firstChannel, int *numChannels)
{
    struct artamd_resampler *hip = cxt->hip;
    if (shard < 0 || shard >= hip->nshards) return -1;
    if (device) *device = hip->shards [shard]->hip->device;
    if (firstChannel) *firstChannel = hip->shard_first [shard];
    if (numChannels) *numChannels = hip->shard_first [shard + 1] - hip->shard_first [shard];
    return 0;
}

void resampleHipSetTiming (Resample *cxt, int enable)
{
    struct artamd_resampler *hip = cxt->hip;
    hip->timing = enable;
    hip->ev_count = 0;
    for (int k = 0; k < hip->nshards; ++k) resampleHipSetTiming (hip->shards [k], enable);
}

/* a sharded context reports its slowest shard (the shards run side by side) */
double resampleHipReadTiming (Resample *cxt, int *numLaunches)
{
    struct artamd_resampler *hip = cxt->hip;
    double total = 0.0;
    if (hip->nshards) {
        int launches = 0;
        for (int k = 0; k < hip->nshards; ++k) {
            int n = 0;
            const double ms = resampleHipReadTiming (hip->shards [k], &n);
            if (ms > total) total = ms;
            if (n > launches) launches = n;
        }
        if (numLaunches) *numLaunches = launches;
        return total;
    }
    ENTER_DEVICE (hip);
    arthip_sync (hip->stream);
    hip->prep_ms = 0.0;
    for (int i = 0; i + 2 < hip->ev_count; i += 3) {         /* (before the launch's first kernel, before its dominant kernel, after it) */
        hip->prep_ms += arthip_event_elapsed_ms (hip->ev [i], hip->ev [i + 1]);
        total += arthip_event_elapsed_ms (hip->ev [i + 1], hip->ev [i + 2]);
    }
    LEAVE_DEVICE (hip);
    if (numLaunches) *numLaunches = hip->ev_count / 3;
    hip->ev_count = 0;
    return total;
}

/* what the launches of the last resampleHipReadTiming spent BEFORE their dominant kernel: the table / staging passes of the
 * matrix-core paths (for the fixed-point kernel: peak pass + digit-plane pass) and the gaps between them */
double resampleHipReadPrepTiming (Resample *cxt)
{
    struct artamd_resampler *hip = cxt->hip;
    double worst = hip->prep_ms;
    for (int k = 0; k < hip->nshards; ++k) {
        const double ms = resampleHipReadPrepTiming (hip->shards [k]);
        if (ms > worst) worst = ms;
    }
    return worst;
}

static void *timing_event (struct artamd_resampler *hip)
{
    if (hip->ev_count == hip->ev_cap) {
        const int cap = hip->ev_cap ? hip->ev_cap * 2 : 96;
        void **grown = realloc (hip->ev, sizeof (void *) * cap);
        if (!grown) return NULL;
        hip->ev = grown;
        for (int i = hip->ev_cap; i < cap; ++i) hip->ev [i] = arthip_event_create ();
        hip->ev_cap = cap;
    }
    return hip->ev [hip->ev_count++];
}

/* a launch's three timing events (before its first kernel — recorded here —, before its dominant kernel, after it: none without timing),
 * and the three given back where the launch enqueued nothing (none of them is read) */
static void take_events (struct artamd_resampler *hip, ArtFirArgs *a)
{
    void *ev_pre = hip->timing ? timing_event (hip) : NULL;
    a->ev_start = hip->timing ? timing_event (hip) : NULL;
    a->ev_stop = hip->timing ? timing_event (hip) : NULL;
    if (ev_pre) arthip_event_record (ev_pre, hip->stream);
}

static void return_events (struct artamd_resampler *hip)
{
    if (hip->timing) hip->ev_count -= 3;
}

/* Did the last call's FIR run on the fixed-point matrix kernel?  0: no; 1: yes; 2: it was enqueued and stood down (a sample
 * outside (-1.98, 1.98) or not finite: the f32 kernel behind it produced the call).  *pairsPerChunk (optional): digit-pair
 * products issued per 32-tap chunk and 32 x 32 outputs, averaged over the tile families (5 .. 13: the products with a digit plane of
 * the rows that is all zero in a chunk — the first away from the rows' centres, the second in the window's tails — are not issued).  Synchronises. */
int resampleHipLastFixedPoint (Resample *cxt, double *pairsPerChunk)
{
    struct artamd_resampler *hip = cxt->hip->nshards ? cxt->hip->shards [0]->hip : cxt->hip;
    if (pairsPerChunk) *pairsPerChunk = 0.0;
    if (!hip->last_fixed [0] || !hip->d_planes) return 0;
    ENTER_DEVICE (hip);
    int flag = 0;
    const int words = hip->last_fixed [1], chunks = hip->last_fixed [2];
    /* (the rows' masks of the first two digit planes, one after the other) */
    unsigned long long *masks = malloc (sizeof (unsigned long long) * (size_t)(words > 0 ? 2 * words : 1));
    arthip_d2h (&flag, hip->d_planes, sizeof (flag), hip->stream);
    if (masks && words > 0) arthip_d2h (masks, hip->last_masks ? hip->last_masks : (void *)((char *) hip->d_planes + ART_I8_HEAD_BYTES), sizeof (unsigned long long) * (size_t)(2 * words), hip->stream);
    arthip_sync (hip->stream);
    if (pairsPerChunk && masks && words > 0 && chunks > 0) {
        double full [2] = { 0.0, 0.0 };
        for (int pl = 0; pl < 2; ++pl)
            for (int v = 0; v < words; v += 32) {             /* a tile family's mask = OR over its 32 rows */
                unsigned long long m = 0;
                for (int r = 0; r < 32; ++r) m |= masks [pl * words + v + r];
                for (; m; m &= m - 1) full [pl] += 1.0;
            }
        /* 5 products with the rows' two lower digit planes always, 4 more per chunk whose second plane is not all zero, 4 more where the first is not */
        *pairsPerChunk = 5.0 + 4.0 * (full [0] + full [1]) / ((double)(words / 32) * chunks);
    }
    free (masks);
    LEAVE_DEVICE (hip);
    return flag == hip->last_fixed [0] ? 2 : 1;
}

/* which form of the fixed-point kernel the last call's last launch was given to (art_hip.h); 0: none */
int resampleHipLastFixedPointKernel (Resample *cxt)
{
    struct artamd_resampler *hip = cxt->hip->nshards ? cxt->hip->shards [0]->hip : cxt->hip;
    return hip->last_fixed [0] ? hip->last_fixed [3] : 0;
}

int  resampleHipLastKernel (Resample *cxt) { return cxt->hip->nshards ? cxt->hip->shards [0]->hip->last_kernel : cxt->hip->last_kernel; }

/* outputs the matrix kernels have evaluated off their canonical pattern so far (synchronises) */
unsigned int resampleHipLastHandedBack (Resample *cxt)
{
    struct artamd_resampler *hip = cxt->hip;
    unsigned int n = 0;
    if (hip->nshards) {
        for (int k = 0; k < hip->nshards; ++k) n += resampleHipLastHandedBack (hip->shards [k]);
        return n;
    }
    if (!hip->d_fix) return 0;
    ENTER_DEVICE (hip);
    arthip_d2h (&n, hip->d_fix + 1, sizeof (n), hip->stream);      /* running total since context creation */
    arthip_sync (hip->stream);
    LEAVE_DEVICE (hip);
    return n;
}


/* ------------------------------------------------------------------------------------------
 * End-point extrapolation (EXTRAPOLATE_ENDPOINTS; reference resampler.c:677-680, :691-698, :812-819).
 * The LPC fits run on the device (extrapolate_kernels.hip), one run per channel, in stream order in front of the call's FIR
 * launches: they read the history ring and the call's input where they lie and write their samples into the ring or d_patch.
 * ---------------------------------------------------------------------------------------- */

/* channel c's `count` frames from linear index `lin` of (history ++ input), as the known samples of a run: the history's frames,
 * then the input's (interleaved, or planar with in_pitch) */
static void linear_run (const Resample *cxt, const art_s *d_in, long in_pitch, int lin, int count, int c, ArtExtrapRun *r)
{
    const struct artamd_resampler *hip = cxt->hip;
    const int C = cxt->numChannels, H = HIST_FRAMES (cxt->numTaps);
    const int from_hist = lin < H ? (H - lin < count ? H - lin : count) : 0, first = lin + from_hist - H;

    r->src [0] = from_hist ? hip->d_hist [hip->cur] + (size_t) lin * C + c : NULL;
    r->stride [0] = C; r->n [0] = from_hist;
    r->src [1] = count > from_hist ? (in_pitch ? d_in + (size_t) c * in_pitch + first : d_in + (size_t) first * C + c) : NULL;
    r->stride [1] = in_pitch ? 1 : C; r->n [1] = count - from_hist;
}

/* Backward extrapolation into the silent pre-history, just before the first output of a stream: the runs of one context
 * (C of them, or 0 when there is nothing to extrapolate from) appended at `runs` */
static int prefill_history_runs (const Resample *cxt, const art_s *d_in, long in_pitch, ArtExtrapRun *runs)
{
    const struct artamd_resampler *hip = cxt->hip;
    const int T = cxt->numTaps, C = cxt->numChannels, H = HIST_FRAMES (T), half = T / 2;
    long first_emit = (long) floor (cxt->outputOffset) + half + 1;     /* inputIndex when output 0 becomes possible */
    if (first_emit < cxt->inputIndex) first_emit = cxt->inputIndex;
    const int known = (int)(first_emit - T), extra = T - known;

    if (known < 8 || extra <= 0) return 0;                              /* reference resampler.c:695 / :815 */

    const int lin_known = T + H - cxt->inputIndex;                      /* ring index T in linear terms */
    for (int c = 0; c < C; ++c) {
        linear_run (cxt, d_in, in_pitch, lin_known, known, c, &runs [c]);
        /* older sample e is ring index T-1-e = linear lin_known-1-e: inside the history buffer by construction */
        runs [c].out = hip->d_hist [hip->cur] + (size_t)(lin_known - 1) * C + c;
        runs [c].out_stride = -C;
        runs [c].extras = extra; runs [c].backward = 1;
    }
    return C;
}

/* Forward extrapolation of half a window at flush time into `tail` (T/2 frames x C): the runs of one context, C of them, at `runs` */
static int flush_tail_runs (const Resample *cxt, art_s *tail, ArtExtrapRun *runs)
{
    const int T = cxt->numTaps, C = cxt->numChannels, H = HIST_FRAMES (T), half = T / 2;
    /* (the reference fits the last T/2 samples and predicts from the last 4: with T = 4 that is 4 samples and no fit, the same) */
    const int known = half < 4 ? 4 : half;

    for (int c = 0; c < C; ++c) {
        linear_run (cxt, NULL, 0, H - known, known, c, &runs [c]);
        runs [c].out = tail + c; runs [c].out_stride = C;
        runs [c].extras = half; runs [c].backward = 0;
    }
    return C;
}

/* The stream's FIRST output is produced by the flush call itself (fewer than T/2 frames ever arrived): the reference's
 * prefill then runs after the postfill (resampler.c:775-791 then :812-819) over the real samples ++ the flush tail.
 * inputIndex is the value BEFORE the flush; the tail (flush_tail_runs, earlier on the stream) is at `tail`.  The runs of one
 * context (C of them, or 0 when there is nothing to extrapolate from) at `runs`. */
static int prefill_at_flush_runs (const Resample *cxt, const art_s *tail, ArtExtrapRun *runs)
{
    const struct artamd_resampler *hip = cxt->hip;
    const int T = cxt->numTaps, C = cxt->numChannels, H = HIST_FRAMES (T), half = T / 2;
    const int real = cxt->inputIndex - T, known = real + half, extra = T - known;

    if (real < 0 || known < 8 || extra <= 0) return 0;                   /* reference resampler.c:695 / :815 */

    for (int c = 0; c < C; ++c) {
        /* ring [T, inputIndex) = the newest `real` history frames, then the tail */
        linear_run (cxt, NULL, 0, H - real, real, c, &runs [c]);
        runs [c].src [1] = tail + c; runs [c].stride [1] = C; runs [c].n [1] = half;
        /* older sample e is ring index T-1-e = linear H - inputIndex + T-1-e = H - real - 1 - e: inside the history */
        runs [c].out = hip->d_hist [hip->cur] + (size_t)(H - real - 1) * C + c;
        runs [c].out_stride = -C;
        runs [c].extras = extra; runs [c].backward = 1;
    }
    return C;
}

static ResampleResult enqueue_call_layouts (Resample *cxt, const art_s *d_in, long in_pitch, int nIn, art_s *d_out, long out_pitch, int cap, double ratio);
static ResampleResult device_call (Resample *cxt, const art_s *d_in, long in_pitch, int nIn, art_s *d_out, long out_pitch, int cap, double ratio);
static ResampleResult peek_call (Resample *cxt, int nIn, int cap, double ratio);
static int staged_layouts (const Resample *cxt, const art_s *d_in, long in_pitch, int nIn, const art_s *d_out, long out_pitch, int cap);
static int rewind_lead (Resample *cxt, int nIn, int cap, double ratio);
static ResampleResult enqueue_call (Resample *cxt, const art_s *d_in, long in_pitch, int nIn,
                                    art_s *d_out, long out_pitch, int cap, double ratio);

/* where a context stands: the planner's state */
static ArtamdPosition position_of (const Resample *cxt)
{
    ArtamdPosition p;
    p.numTaps = cxt->numTaps; p.numFilters = cxt->numFilters; p.flags = cxt->flags; p.inputIndex = cxt->inputIndex;
    p.floorActive = cxt->hip->floor_active; p.outputOffset = cxt->outputOffset; p.fixedRatio = cxt->fixedRatio;
    return p;
}

/* plan a call from the context's position into hip->segs, grown as needed (*trial: the position after the call); returns the segment count,
 * -1 out of memory */
static int plan_segments (Resample *cxt, int nIn, int cap, double ratio, ArtamdPosition *trial, ResampleResult *res, int *lin_floor)
{
    struct artamd_resampler *hip = cxt->hip;
    for (;;) {
        *trial = position_of (cxt);
        const int nseg = artamdPlanCall (trial, nIn, cap, ratio, res, hip->segs, hip->seg_cap, lin_floor);
        if (nseg <= hip->seg_cap) return nseg;
        ArtamdSegment *grown = realloc (hip->segs, sizeof (ArtamdSegment) * (size_t)(nseg + 16));
        if (!grown) return -1;
        hip->segs = grown; hip->seg_cap = nseg + 16;
    }
}

/* One context's call, planned: what the single call, the batch entries and the schedule all derive from the context and the call's
 * arguments before anything is enqueued.  The segments themselves are in hip->segs until the context's next plan. */
typedef struct {
    ArtamdPosition trial;                    /* the position after the call */
    ResampleResult res;                      /* the call's counts */
    int nseg, lin_floor;
    int is_flush, appended;                  /* a flush appends half a window (its tail, or silence) to the history, any other call the input it used */
    /* the EXTRAPOLATE_ENDPOINTS fits due in front of the FIR launches */
    int fit_prefill;                         /* backwards from (history ++ input), just before the stream's first output */
    int fit_tail;                            /* forwards, the flush's half window */
    int fit_late;                            /* backwards from the samples ++ that tail: the flush itself makes the first output */
} CallPlan;

/* returns the segment count, -1 out of memory */
static int plan_one_call (Resample *cxt, int nIn, int cap, double ratio, CallPlan *p)
{
    const int T = cxt->numTaps;
    p->is_flush = nIn < 0 && !(cxt->flags & RESAMPLER_FLUSHED);
    p->nseg = plan_segments (cxt, nIn, cap, ratio, &p->trial, &p->res, &p->lin_floor);
    if (p->nseg < 0) return -1;
    p->appended = p->is_flush ? T / 2 : (int) p->res.input_used;
    /* the prefill comes just before the first output of the stream (resampler.c:812-819), whichever call produces it: an ordinary call (a
     * rewind right in front of output 0 leaves one known sample: nothing to extrapolate from), a flush continued after it was cut short, or
     * the flush call itself (one that had to rewind the ring first leaves more than T known samples: nothing to prefill) */
    const int first = (cxt->flags & EXTRAPOLATE_PREFILL) && p->res.output_generated;
    p->fit_prefill = first && !p->is_flush && (p->nseg == 1 || cxt->hip->segs [1].first_output > 0);
    p->fit_tail = p->is_flush && (cxt->flags & EXTRAPOLATE_ENDPOINTS);
    p->fit_late = p->fit_tail && first && p->trial.inputIndex == cxt->inputIndex + T / 2;
    return p->nseg;
}

/* segments [s0, s1) of the planned call as a launch's table */
static void seg_table (const struct artamd_resampler *hip, int s0, int s1, int lin_floor, ArtSegTable *tab)
{
    tab->count = s1 - s0; tab->lin_floor = lin_floor;
    for (int s = s0; s < s1; ++s) {
        tab->first [s - s0] = hip->segs [s].first_output;
        tab->lin_base [s - s0] = hip->segs [s].lin_base;
        tab->base [s - s0] = hip->segs [s].base_offset;
    }
}

/* the call's FIR arguments, and the rational structure of its ratio (the launches' outputs, tables and buffers are the caller's) */
static void fill_args (Resample *cxt, ArtFirArgs *a, double ratio, const art_s *in, long in_pitch, int in_frames, art_s *out, long out_pitch)
{
    struct artamd_resampler *hip = cxt->hip;
    const double eff_ratio = (cxt->flags & RESAMPLE_FIXED_RATIO) ? cxt->fixedRatio : ratio;
    if (eff_ratio != hip->period_ratio) {
        hip->period_ratio = eff_ratio;
        find_period (eff_ratio, &hip->period_out, &hip->period_in);
    }
    memset (a, 0, sizeof (*a));
    a->bank = hip->d_bank; a->hist = hip->d_hist [hip->cur];
    a->in = in; a->in_pitch = in_pitch; a->in_frames = in_frames;
    a->out = out; a->out_pitch = out_pitch;
    a->C = cxt->numChannels; a->T = cxt->numTaps; a->F = cxt->numFilters; a->H = HIST_FRAMES (cxt->numTaps);
    a->stream_C = hip->stream_channels;
    a->lin_origin = hip->lin_origin;
    a->interpolate = (cxt->flags & SUBSAMPLE_INTERPOLATE) != 0;
    a->lowpass = (cxt->flags & INCLUDE_LOWPASS) != 0;
    /* the double-precision build has one arithmetic: EXTEND_CONVOLUTION_MATH only matters for 4-byte samples
     * (reference resampler.c:191) */
    const int extend = !ART_WIDE && (cxt->flags & EXTEND_CONVOLUTION_MATH);
    a->mode = (cxt->flags & RESAMPLE_STRICT_ORDER) ? ART_MODE_STRICT : extend ? ART_MODE_PRECISE : ART_MODE_FAST;
    if ((cxt->flags & RESAMPLE_STRICT_ORDER) && extend) a->mode |= 4;
    a->ratio = eff_ratio;
    a->period_out = hip->period_out; a->period_in = hip->period_in;
}

/* A planned call as ONE launch with its first table: every output, the history roll riding along.  A flush reads its extrapolated `tail`
 * (T/2 frames) or, without one (NULL), no input frames at all: silence. */
static void plan_args (Resample *cxt, const CallPlan *p, double ratio, const art_s *in, long in_pitch, art_s *out, long out_pitch, const art_s *tail,
                       ArtFirArgs *a, ArtSegTable *tab)
{
    struct artamd_resampler *hip = cxt->hip;
    if (p->is_flush) fill_args (cxt, a, ratio, tail, 0, tail ? cxt->numTaps / 2 : 0, out, out_pitch);
    else fill_args (cxt, a, ratio, in, in_pitch, (int) p->res.input_used, out, out_pitch);
    seg_table (hip, 0, p->nseg < ART_MAX_SEGS ? p->nseg : ART_MAX_SEGS, p->lin_floor, tab);
    a->n_begin = hip->segs [0].first_output; a->n_end = p->res.output_generated;
    a->roll_dst = p->appended > 0 ? hip->d_hist [hip->cur ^ 1] : NULL;
    a->roll_appended = p->appended;
}

/* The fits due for a planned call, appended to the caller's lists: `late` reads what `early` writes (the flush's tail, T/2 x C frames at
 * `tail`) and so is a second launch */
static void plan_fits (const Resample *cxt, const CallPlan *p, const art_s *in, long in_pitch, art_s *tail,
                       ArtExtrapRun *early, int *nearly, ArtExtrapRun *late, int *nlate)
{
    if (p->fit_prefill) *nearly += prefill_history_runs (cxt, in, in_pitch, early + *nearly);
    if (p->fit_tail) *nearly += flush_tail_runs (cxt, tail, early + *nearly);
    if (p->fit_late) *nlate += prefill_at_flush_runs (cxt, tail, late + *nlate);
}

/* ... of the single call, launched on its stream (the tail in d_patch); 0 or -1 */
static int launch_fits (Resample *cxt, const CallPlan *p, const art_s *in, long in_pitch)
{
    struct artamd_resampler *hip = cxt->hip;
    const int C = cxt->numChannels;
    ArtExtrapRun *runs = malloc (sizeof (ArtExtrapRun) * 2 * (size_t) C);      /* (C early, C late at most) */
    int nearly = 0, nlate = 0, rc = -1;

    if (p->fit_tail) hip->d_patch = arthip_grow (hip->d_patch, &hip->patch_cap, sizeof (art_s) * (size_t)(cxt->numTaps / 2) * C);
    if (runs && (hip->d_patch || !p->fit_tail)) {
        plan_fits (cxt, p, in, in_pitch, hip->d_patch, runs, &nearly, runs + C, &nlate);
        rc = (nearly && arthip_extrapolate (runs, nearly, hip->stream)) || (nlate && arthip_extrapolate (runs + C, nlate, hip->stream)) ? -1 : 0;
    }
    free (runs);
    return rc;
}

/* the canonical period of the rows the matrix kernels keep across calls: looked after by every launch of a rational-ratio stream,
 * whichever kernel runs it (fir_matrix.hip, artfir_rows_touch) — not by a flush's */
static void keep_rows (struct artamd_resampler *hip, ArtFirArgs *a)
{
    if (a->period_out && a->mode == ART_MODE_FAST && !hip->rows_off) {
        if (!hip->rows_cache && arthip_fir_rows_cache_bytes ()) hip->rows_cache = calloc (1, arthip_fir_rows_cache_bytes ());
        a->rows_cache = hip->rows_cache;
    }
}

/* grow a device buffer; a new one starts with its first `head` bytes zero */
static void *grow_zeroed (void *dev, size_t *cap, size_t need, size_t head, void *stream)
{
    if (need <= *cap) return dev;
    dev = arthip_grow (dev, cap, need);
    if (dev) arthip_zero (dev, head, stream);
    return dev;
}

/* The buffers a call's matrix-core launches need (arthip_fir_needs), handed to them in *a: allocated only once a call of this context is
 * actually big enough for them (a service with thousands of small-block contexts never pays for them).  Returns 1 when the path has its
 * counters and scratch; a failed allocation leaves the call on the general kernel. */
static int provision (struct artamd_resampler *hip, const ArtFirNeeds *n, ArtFirArgs *a)
{
    hip->last_fixed [0] = 0;
    if (!n->matrix) return 0;
    /* [0] per-launch count, [1] running total of outputs the matrix kernels evaluated off their canonical pattern
     * (diagnostics only: they are computed inside the kernel) */
    hip->d_fix = grow_zeroed (hip->d_fix, &hip->fix_cap, 64, 2 * sizeof (unsigned int), hip->stream);
    if (hip->d_fix) { a->fix_count = hip->d_fix; a->fix_list = hip->d_fix + 2; a->fix_cap = 0; }
    hip->d_scratch = arthip_grow (hip->d_scratch, &hip->scratch_cap, n->scratch_bytes);
    a->scratch = hip->d_scratch; a->scratch_bytes = hip->d_scratch ? hip->scratch_cap : 0;
    /* digit planes for the fixed-point kernel (about the size of the call's input; without them the f32 kernels run) */
    hip->d_planes = grow_zeroed (hip->d_planes, &hip->planes_cap, n->planes_bytes, ART_I8_HEAD_BYTES, hip->stream);
    a->planes = n->planes_bytes ? hip->d_planes : NULL; a->planes_bytes = hip->d_planes ? hip->planes_cap : 0;
    /* ... and the matrix kernels' filter rows, which outlive the call: built by the first launch of a stream, looked up by the others
     * (none without their host block: resampleHipKeepRows (0), the 8-byte build) */
    const size_t rows_want = a->rows_cache ? n->rows_bytes : 0;
    if (rows_want > hip->rows_cap) {
        hip->d_rows = arthip_grow (hip->d_rows, &hip->rows_cap, rows_want);
        arthip_fir_rows_cache_reset (hip->rows_cache);
    }
    if (rows_want && hip->d_rows) { a->rows = hip->d_rows; a->rows_bytes = hip->rows_cap; }
    hip->last_masks = NULL; a->rows_masks_out = &hip->last_masks;
    /* calls of few tiles: room for the K-split kernel's partial sums (a grown buffer starts with its counters zeroed; the
     * old one is released behind the launches that used it: stream order) */
    hip->d_split = grow_zeroed (hip->d_split, &hip->split_cap, n->split_bytes, ART_SPLIT_HEAD_BYTES, hip->stream);
    a->split = n->split_bytes ? hip->d_split : NULL; a->split_bytes = hip->d_split ? hip->split_cap : 0;
    a->fixed_out = hip->last_fixed;
    /* a channel count the matrix kernels are not compiled for: room for its groups' padded copies */
    hip->d_pad = arthip_grow (hip->d_pad, &hip->pad_cap, n->pad_bytes);
    a->pad = n->pad_bytes ? hip->d_pad : NULL; a->pad_bytes = hip->d_pad ? hip->pad_cap : 0;
    return a->fix_list && a->scratch;
}

/* EXTRAPOLATE_ENDPOINTS, first output of the stream only after the ring has rewound (the position was advanced by more than 15 T):
 * the reference extrapolates backwards from the samples that arrived SINCE the rewind, over the history (resampler.c:812-819 with
 * the ring's inputIndex).  The single call then consumes the frames before the one that makes output 0 possible silently first
 * (consume_silently); the rest of the call starts inside the right ring epoch and prefills as usual.  Returns how many frames
 * that is, or 0 where an ordinary (non-flush) call of nIn frames takes no such route. */
static int rewind_lead (Resample *cxt, int nIn, int cap, double ratio)
{
    ResampleResult one;
    int lin_floor;
    if (!(cxt->flags & EXTRAPOLATE_PREFILL) || nIn <= 1 || cap <= 0 || (cxt->flags & RESAMPLER_FLUSHED)) return 0;
    ArtamdPosition trial = position_of (cxt);
    if (plan_call (&trial, nIn, 1, ratio, &one, NULL, 0, &lin_floor, 1) >= 2 && one.output_generated == 1 && one.input_used >= 2)
        return (int) one.input_used - 1;
    return 0;
}

/* A call's launches are enqueued: the context moves to the planned position (the prefill stays due until a call has made output), and
 * the history ring to the buffer the roll wrote */
static void commit_position (Resample *cxt, const ArtamdPosition *trial, int made_output)
{
    cxt->outputOffset = trial->outputOffset; cxt->inputIndex = trial->inputIndex;
    cxt->flags = (cxt->flags & ~(RESAMPLER_FLUSHED | EXTRAPOLATE_PREFILL)) | (trial->flags & RESAMPLER_FLUSHED) |
                 (made_output ? 0 : (cxt->flags & EXTRAPOLATE_PREFILL));
    cxt->hip->floor_active = trial->floorActive;
}

static void commit_history (struct artamd_resampler *hip, int appended)
{
    if (appended > 0) { hip->cur ^= 1; hip->lin_origin += appended; }
}

/* nothing consumed, nothing made: results [k], or with `owner` results [owner [k]], k < n */
static void zero_results (ResampleResult *results, const int *owner, int n)
{
    for (int k = 0; k < n; ++k) {
        ResampleResult *r = &results [owner ? owner [k] : k];
        r->input_used = r->output_generated = 0;
    }
}

/* The first `frames` input frames of a call go into the history without any output being due (the caller established
 * that): position and ring epoch advance exactly as the reference's loop would have advanced them. */
static int consume_silently (Resample *cxt, const art_s *d_in, long in_pitch, int frames, double ratio)
{
    struct artamd_resampler *hip = cxt->hip;
    const int T = cxt->numTaps, C = cxt->numChannels, H = HIST_FRAMES (T);
    ArtamdPosition pos = position_of (cxt);
    ResampleResult res;
    int lin_floor;

    plan_call (&pos, frames, 1, ratio, &res, NULL, 0, &lin_floor, 1);
    if (res.output_generated || (int) res.input_used != frames) return -1;

    if (arthip_roll_history (hip->d_hist [hip->cur ^ 1], hip->d_hist [hip->cur], d_in, in_pitch, frames, H, C, hip->stream)) return -1;
    commit_history (hip, frames);
    commit_position (cxt, &pos, 0);
    return 0;
}

/* Plan one call, enqueue the FIR launches and the history roll.  `d_in` holds the call's input on
 * the device (interleaved, or planar with `in_pitch`); `d_out` receives the output likewise. */
static ResampleResult enqueue_call (Resample *cxt, const art_s *d_in, long in_pitch, int nIn,
                                    art_s *d_out, long out_pitch, int cap, double ratio)
{
    struct artamd_resampler *hip = cxt->hip;
    const int C = cxt->numChannels, H = HIST_FRAMES (cxt->numTaps);
    CallPlan p;
    ArtFirArgs a;
    ArtSegTable tab;
    int lead, rolled = 0;

    hip->last_gathered = 0;
    /* EXTRAPOLATE_ENDPOINTS, first output of the stream only after the ring has rewound: consumed silently up to it (rewind_lead) */
    if ((lead = rewind_lead (cxt, nIn, cap, ratio)) > 0) {
        ResampleResult res = { 0, 0 };
        if (consume_silently (cxt, d_in, in_pitch, lead, ratio)) {
            fprintf (stderr, "artamd: end-point extrapolation: could not advance to the first output: %s\n", arthip_last_error ());
            return res;
        }
        res = enqueue_call (cxt, in_pitch ? d_in + lead : d_in + (size_t) lead * C, in_pitch, nIn - lead, d_out, out_pitch, cap, ratio);
        res.input_used += (unsigned int) lead;
        return res;
    }

    const int nseg = plan_one_call (cxt, nIn, cap, ratio, &p);
    /* (a failure from here on: nothing of the stream has moved — the position and the history ring are committed below, behind the call's
     * last launch —, a caller sees { 0, 0 }, the count in artamdErrorCount, and with ARTAMD_ABORT_ON_ERROR=1 the process stops there) */
    const char *failure = nseg < 0 ? "resampler: out of memory (segment table)" : NULL;
    if (!failure && (p.fit_prefill || p.fit_tail) && launch_fits (cxt, &p, d_in, in_pitch))
        failure = "resampler: end-point extrapolation launch failed";
    if (failure) goto failed;

    plan_args (cxt, &p, ratio, d_in, in_pitch, d_out, out_pitch, p.fit_tail ? hip->d_patch : NULL, &a, &tab);
    if (p.res.output_generated) {
        if (!p.is_flush) keep_rows (hip, &a);
        /* what the call's launches need (a flush runs on the general kernel) */
        ArtFirNeeds needs;
        memset (&needs, 0, sizeof (needs));
        if (!p.is_flush) arthip_fir_needs (&a, &tab, p.res.output_generated, hip->kernel_pref, &needs);
        const int matrix = provision (hip, &needs, &a);

        /* A call of more ring epochs than a table holds (short filters: an epoch is a few hundred frames) is cut into launches of
         * ART_MAX_SEGS segments — unless it runs on a streaming matrix-core kernel, which follows the lattice from its first period
         * and needs the table for that period only: then the whole call is ONE launch with the first table (a launch that declines
         * after all enqueues nothing and the cut launches follow) */
        int whole = matrix && nseg > ART_MAX_SEGS && needs.one_launch;
        for (int s0 = 0; s0 < nseg; s0 += ART_MAX_SEGS) {
            const int s_tab = s0 + ART_MAX_SEGS < nseg ? s0 + ART_MAX_SEGS : nseg;     /* segments in this launch's table ... */
            const int s1 = whole ? nseg : s_tab;                                       /* ... and those it produces */

            if (s0) seg_table (hip, s0, s_tab, p.lin_floor, &tab);                     /* (the first is the plan's) */
            a.n_begin = hip->segs [s0].first_output;
            a.n_end = s1 < nseg ? hip->segs [s1].first_output : p.res.output_generated;
            if (a.n_end > a.n_begin) {
                take_events (hip, &a);
                /* the last FIR launch of the call may take the history roll along (one launch less on the stream) */
                a.roll_dst = (s1 == nseg && p.appended > 0) ? hip->d_hist [hip->cur ^ 1] : NULL;
                a.segs_truncated = whole;
                int k = arthip_fir (&a, &tab, hip->kernel_pref, hip->stream);
                a.segs_truncated = 0;
                if (k == -2 && whole) {                /* (declined: nothing enqueued — again, cut) */
                    return_events (hip);
                    whole = 0; s0 = -ART_MAX_SEGS; continue;
                }
                if (k >= 0 && (k & ART_FIR_ROLLED)) { rolled = 1; k &= ~ART_FIR_ROLLED; }
                if (k < 0) { failure = "resampler: FIR launch failed"; goto failed; }
                hip->last_kernel = k;
                /* the cut-invariant policy: a launch of a rational-ratio stream that could not run anchored on the matrix cores went to the general
                 * kernel — still independent of the cut by itself, but another arithmetic than the stream's other outputs: counted (art_hip.h) */
                if (hip->kernel_pref == ART_KERNEL_INVARIANT && k == ART_KERNEL_GENERAL && a.period_out && a.mode == ART_MODE_FAST && !p.is_flush)
                    hip->invariant_fallbacks++;
            }
            if (whole) break;
        }
    }

    if (p.appended > 0 && !rolled)
        arthip_roll_history (hip->d_hist [hip->cur ^ 1], hip->d_hist [hip->cur], a.in, a.in_pitch, p.appended, H, C, hip->stream);
    commit_history (hip, p.appended);
    commit_position (cxt, &p.trial, p.res.output_generated != 0);
    return p.res;

failed:
    artamd_note_failure (failure);
    zero_results (&p.res, NULL, 1);
    return p.res;
}

/* ---- many independent streams, one launch -------------------------------------------------------------------------
 * A service that resamples hundreds of streams in small blocks is launch-bound one call at a time.  This entry point
 * plans every context's call on the host exactly as the single call does, gathers those the general kernel would run
 * (any ratio per stream, default or EXTEND mode, ordinary call, on the stream of cxts [0]) into one launch per kernel
 * variant — each stream cut into the tiles its own launch would use, so the samples are identical — gathers those the single call
 * would make as one un-split launch of the f32 streaming matrix-core kernel on rows kept across calls (calls big enough for that path,
 * every anchored call of a context under the cut-invariant policy) into one launch per shape (arthip_fir_group: the tiles of every
 * such launch, unchanged, on one grid), and simply makes the remaining calls (flushes, strict mode, matrix-core calls of any other
 * kind — a stream's first, which builds its rows, the fixed-point and K-split kernels', channel counts without a compiled width —,
 * other streams, a first output after a rewind) one by one.  The first output of an extrapolating stream is gathered
 * too: its backward fits, for all such streams, are one launch in front of the FIR launches.  results [i] is what
 * resampleProcessInterleavedDevice (cxts [i], ...) would have returned. */
/* May a context's call be gathered with others (batched streams, scheduled blocks)?  Not a sharded context's, and neither in strict order
 * nor on a flushed stream (those calls are made as they stand); a call that may bring fits — the flush of an extrapolating stream, an ordinary
 * call before such a stream's first output (after it, its ordinary calls are a plain stream's) — only where there is room for their runs */
static int gatherable (const Resample *cxt, int is_flush, int have_runs)
{
    if (cxt->hip->nshards || (cxt->flags & (RESAMPLE_STRICT_ORDER | RESAMPLER_FLUSHED))) return 0;
    return have_runs || !(cxt->flags & (is_flush ? EXTRAPOLATE_ENDPOINTS : EXTRAPOLATE_PREFILL));
}

/* Does the single call give this planned call (its FIR arguments, first table, outputs) to the general kernel?  The cut-invariant policy keeps
 * a rational-ratio stream's calls for itself (every launch anchored on the stream's canonical period, or counted where it cannot be: the
 * single call decides that, with the context's kept rows); a call big enough for the matrix-core path is that path's (the same question the
 * single call asks) */
static int general_call (const Resample *cxt, const ArtFirArgs *a, const ArtSegTable *first, unsigned int outputs)
{
    const struct artamd_resampler *hip = cxt->hip;
    if (hip->kernel_pref == ART_KERNEL_INVARIANT && a->period_out && a->mode == ART_MODE_FAST) return 0;
    ArtFirNeeds needs;
    arthip_fir_needs (a, first, outputs, hip->kernel_pref, &needs);
    return !needs.matrix;
}

/* Where a batch call's context reads and writes: the caller's buffers with their pitches (0: interleaved), or — a planar call the single call
 * would stage (staged_layouts) — the context's own interleaved staging, filled and emptied by the batch's two transposing launches.
 * staged < 0: the transposing launch in front could not be made, the call is the single planar call on the caller's buffers. */
typedef struct { const art_s *in; art_s *out; long in_pitch, out_pitch; int staged; } BatchIo;

/* What a batch call has gathered.  For the general kernel's launch: the FIR arguments, first table and plan of each gathered call (`owner`: its
 * index in the caller's list), and the extrapolation runs in front of it — `runs`, and `late`, which read what `runs` write (a flush: the
 * prefill of a stream whose first output the flush makes reads the tails) and so are a second launch.  For the grouped matrix-core launches: the
 * planned launch (arthip_fir_group_plan), plan and owner of each call (`calls` NULL: no room, such calls are made one by one). */
typedef struct {
    ArtFirArgs *args; ArtSegTable *tabs; CallPlan *plans; int *owner; int gathered;
    ArtFirGroupCall *calls; CallPlan *matrix_plans; int *matrix_owner; int matrix_gathered;
    ArtExtrapRun *runs, *late; int nruns, nlate;
} BatchWork;

/* A grouped matrix-core launch has at least this many calls; the calls of a smaller class are made one by one (a class of one: no table
 * upload for nothing) */
#define MATRIX_GROUP_MIN 2

/* room for n calls on either list (`matrix` 0: none on the second) and run_cap runs of either kind (0: none — extrapolating calls are then made
 * one by one); 0 or -1 */
static int batch_work_init (BatchWork *w, int n, size_t run_cap, int matrix)
{
    memset (w, 0, sizeof (*w));
    w->args = malloc (sizeof (ArtFirArgs) * (size_t) n); w->tabs = malloc (sizeof (ArtSegTable) * (size_t) n);
    w->plans = malloc (sizeof (CallPlan) * 2 * (size_t) n); w->owner = malloc (sizeof (int) * 2 * (size_t) n);
    if (!w->args || !w->tabs || !w->plans || !w->owner) return -1;
    w->matrix_plans = w->plans + n; w->matrix_owner = w->owner + n;
    if (matrix) w->calls = malloc (sizeof (ArtFirGroupCall) * (size_t) n);
    if (run_cap && (w->runs = malloc (sizeof (ArtExtrapRun) * 2 * run_cap)) != NULL) w->late = w->runs + run_cap;
    return 0;
}

static void batch_work_free (BatchWork *w)
{
    free (w->args); free (w->tabs); free (w->plans); free (w->owner); free (w->calls); free (w->runs);
}

/* The planned call is not the general kernel's: may it run in a grouped matrix-core launch?  As the single call goes about it — the context's
 * kept rows, what the launch needs, its buffers — up to the launch itself, which is only planned (1: at w's next matrix place); 0: the single call's */
static int batch_plan_matrix (Resample *cxt, ArtFirArgs *a, const ArtSegTable *tab, const CallPlan *p, BatchWork *w)
{
    struct artamd_resampler *hip = cxt->hip;
    ArtFirNeeds needs;
    if (ART_WIDE || !w->calls) return 0;
    keep_rows (hip, a);
    arthip_fir_needs (a, tab, p->res.output_generated, hip->kernel_pref, &needs);
    /* (a call of more segments than its table holds: one launch only where the single call would try that first) */
    if (!needs.matrix || (p->nseg > ART_MAX_SEGS && !needs.one_launch) || !provision (hip, &needs, a)) return 0;
    a->segs_truncated = p->nseg > ART_MAX_SEGS;
    if (!arthip_fir_group_plan (a, tab, hip->kernel_pref, &w->calls [w->matrix_gathered])) return 0;
    w->matrix_plans [w->matrix_gathered] = *p;
    return 1;
}

/* Plan one context's call as the single call would; gather it at w's next place (1) if the general kernel is the single call's and the
 * context may share a launch, at w's next matrix place (2) if a grouped matrix-core launch may run it, else leave the context as it stands
 * (0: the caller makes the single call).
 * The buffers are interleaved, or planar where a pitch is given (the general kernel, the history rolls and the fits read and write planes as they
 * come).
 * nIn >= 0, an ordinary call: an extrapolating stream's first output brings its prefill runs, as the single call would make them.
 * nIn < 0, a flush: `tail` is room for the context's T/2 x C tail frames when it extrapolates (NULL: none, the flush is the single call).
 * The flush proper runs on the general kernel whatever the context's other calls run on; it brings its forward tail fits (w->runs) and,
 * when it makes the stream's first output, the prefill over the samples ++ the tail (w->late).  (The flush call of an already flushed
 * stream is the single call: behind the process phase it has no output left to make.) */
static int batch_plan (Resample *cxt, const art_s *d_in, long in_pitch, int nIn, art_s *d_out, long out_pitch, int cap, double ratio, void *lead_stream,
                       art_s *tail, BatchWork *w)
{
    struct artamd_resampler *hip = cxt->hip;
    ArtFirArgs *a = &w->args [w->gathered];
    ArtSegTable *tab = &w->tabs [w->gathered];
    CallPlan *p = &w->plans [w->gathered];
    const int is_flush = nIn < 0;

    if (hip->stream != lead_stream || hip->timing || hip->device != arthip_current_device ()) return 0;
    /* (a first output after a rewind is the single call's, which consumes the frames in front of it silently) */
    if (!gatherable (cxt, is_flush, w->runs && (tail || !is_flush)) || rewind_lead (cxt, nIn, cap, ratio)) return 0;

    /* (out of memory: the one-by-one path reports it; a flush without an output still appends its half window to the history: an item of
     * roll workgroups only) */
    if (plan_one_call (cxt, nIn, cap, ratio, p) < 0 || (p->res.output_generated == 0 && !is_flush)) return 0;
    plan_args (cxt, p, ratio, d_in, in_pitch, d_out, out_pitch, p->fit_tail ? tail : NULL, a, tab);
    /* (the matrix-core path takes interleaved frames only: a planar call that is not the general kernel's is the single call's to decide) */
    if (!is_flush && !general_call (cxt, a, tab, p->res.output_generated))
        return !in_pitch && !out_pitch && !(cxt->flags & EXTRAPOLATE_PREFILL) && batch_plan_matrix (cxt, a, tab, p, w) ? 2 : 0;
    /* (the general kernel's gathered launch takes calls of a few segments; the matrix-core path's follows the lattice from the first table) */
    if (p->nseg > arthip_fir_batch_max_segments ()) return 0;
    /* (... and calls whose span fits the launch's LDS budget: a ratio below that is the single call's, as a schedule's block of that kind is) */
    if (!arthip_fir_batch_accepts (a)) return 0;
    plan_fits (cxt, p, d_in, in_pitch, tail, w->runs, &w->nruns, w->late, &w->nlate);
    return 1;
}

/* the gathered calls' launches on the lead's stream: the fits, those that read them, then every FIR (the history rolls ride along); 0 or -1 */
static int batch_launch (struct artamd_resampler *lead, const BatchWork *w)
{
    lead->d_batch = arthip_grow (lead->d_batch, &lead->batch_cap, arthip_fir_batch_item_bytes () * (size_t) w->gathered);
    if (lead->d_batch && !(w->nruns && arthip_extrapolate (w->runs, w->nruns, lead->stream)) &&
        !(w->nlate && arthip_extrapolate (w->late, w->nlate, lead->stream)) &&
        !arthip_fir_batch (w->args, w->tabs, w->gathered, lead->d_batch, lead->stream))
        return 0;
    fprintf (stderr, "artamd: resample batch launch failed: %s\n", arthip_last_error ());
    return -1;
}

/* ... and the contexts' positions and histories, behind them */
static void batch_commit (Resample *const *cxts, const CallPlan *plans, const int *owner, int n, int kernel)
{
    for (int k = 0; k < n; ++k) {
        Resample *cxt = cxts [owner [k]];
        const int made_output = plans [k].res.output_generated != 0;
        cxt->hip->last_gathered = 1;
        commit_history (cxt->hip, plans [k].appended);
        commit_position (cxt, &plans [k].trial, made_output);
        if (made_output) cxt->hip->last_kernel = kernel;
    }
}

/* The calls planned for grouped matrix-core launches: classes by shape; the calls of a class too small for a launch of its own are made one by
 * one (the contexts stand where they stood), the others launched — one launch per class — and committed.  0, or -1: the grouped launches failed
 * (nothing of them enqueued: their contexts' results { 0, 0 }, positions and histories untouched; counted, artamdErrorCount: -2). */
static int batch_matrix (Resample *const *cxts, BatchWork *w, const BatchIo *io, const int *numInputFrames, const int *numOutputFrames,
                         const double *ratios, ResampleResult *results)
{
    struct artamd_resampler *lead = cxts [0]->hip;
    ArtFirGroupCall *calls = w->calls;
    const int n = w->matrix_gathered;
    int *rep = malloc (sizeof (int) * 2 * (size_t) n), *count = rep ? rep + n : NULL;      /* a class's first call, its size */
    int classes = 0, kept = 0, rc = 0;
    if (!rep) {
        for (int k = 0; k < n; ++k) calls [k].cls = -1;
    }
    else for (int k = 0; k < n; ++k) {
        int c = 0;
        while (c < classes && !arthip_fir_group_same_class (&calls [rep [c]], &calls [k])) ++c;
        if (c == classes) { rep [classes] = k; count [classes++] = 0; }
        calls [k].cls = c; ++count [c];
    }
    /* the classes that are launched, renumbered 0 ..; their calls moved to the front */
    for (int c = 0, next = 0; c < classes; ++c) rep [c] = count [c] >= MATRIX_GROUP_MIN ? next++ : -1;
    for (int k = 0; k < n; ++k) {
        const int i = w->matrix_owner [k], c = calls [k].cls < 0 ? -1 : rep [calls [k].cls];
        if (c < 0) { results [i] = device_call (cxts [i], io [i].in, 0, numInputFrames [i], io [i].out, 0, numOutputFrames [i], ratios [i]); continue; }
        calls [kept] = calls [k]; calls [kept].cls = c; w->matrix_plans [kept] = w->matrix_plans [k]; w->matrix_owner [kept++] = i;
    }
    free (rep);
    if (kept) {
        lead->d_group = arthip_grow (lead->d_group, &lead->group_cap, arthip_fir_group_table_bytes (kept));
        if (!lead->d_group || arthip_fir_group (calls, kept, lead->d_group, lead->stream)) {
            fprintf (stderr, "artamd: resample batch: grouped matrix-core launch failed: %s\n", arthip_last_error ());
            artamd_note_failure ("resampler: grouped FIR launch failed");
            zero_results (results, w->matrix_owner, kept);
            rc = -2;                     /* (counted) */
        }
        else batch_commit (cxts, w->matrix_plans, w->matrix_owner, kept, ART_KERNEL_MFMA);
    }
    return rc;
}

static unsigned long *stamp_of (const void *cxt) { return &((const Resample *) cxt)->hip->batch_stamp; }

/* May a context's planar call be staged by the batch's own transposing launches?  They run on the lead's stream: a context the batch makes one by
 * one anyway (sharded, another stream or device, timing on) stages its call itself, as the single planar call does */
static int shares_lead (const Resample *cxt, const struct artamd_resampler *lead)
{
    const struct artamd_resampler *hip = cxt->hip;
    return !hip->nshards && hip->stream == lead->stream && !hip->timing && hip->device == lead->device;
}

/* one transposing launch over the staged calls of a batch (the table in the lead's d_layout: `slot` 0 in front of the FIR launches, 1 behind) */
static int batch_transpose (struct artamd_resampler *lead, ArtLayoutItem *items, int count, int n, int to_planar)
{
    if (!count) return 0;
    lead->d_layout = arthip_grow (lead->d_layout, &lead->layout_cap, sizeof (ArtLayoutItem) * 2 * (size_t) n);
    if (lead->d_layout && !arthip_transpose_group (items, count, to_planar, (ArtLayoutItem *) lead->d_layout + (to_planar ? n : 0), lead->stream)) return 0;
    fprintf (stderr, "artamd: resample batch: transposing launch failed: %s\n", arthip_last_error ());
    return -1;
}

/* the batch entries' process phase, on the lead's device: every context's ordinary call, gathered or single.  Pitches as in
 * resampleProcessPlanarDevice (NULL: every buffer of that side interleaved).  A planar call decides as the single planar call does
 * (staged_layouts): left as it is, it is the general kernel's with its pitches; staged, it is the interleaved call on the context's own
 * staging — all such calls' inputs transposed by one launch in front of everything else, their outputs by one launch behind. */
static int batch_process (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const long *in_pitches, const int *numInputFrames,
                          artsample_t *const *d_outputs, const long *out_pitches, const int *numOutputFrames, const double *ratios,
                          ResampleResult *results, BatchIo *io)
{
    struct artamd_resampler *lead = cxts [0]->hip;
    BatchWork w;
    ArtLayoutItem *items = NULL;
    int rc = -1, failed = 0, staged = 0, moved = 0;

    size_t channels = 0;                 /* (room for the prefill runs of every extrapolating stream's first output: one per channel) */
    for (int i = 0; i < n; ++i)
        if ((cxts [i]->flags & EXTRAPOLATE_PREFILL) && !cxts [i]->hip->nshards) channels += (size_t) cxts [i]->numChannels;
    if (batch_work_init (&w, n, channels, 1)) goto out;

    for (int i = 0; i < n; ++i) {
        Resample *cxt = cxts [i];
        struct artamd_resampler *hip = cxt->hip;
        BatchIo *b = &io [i];
        b->in = d_inputs [i]; b->out = d_outputs [i]; b->staged = 0;
        b->in_pitch = in_pitches ? in_pitches [i] : 0; b->out_pitch = out_pitches ? out_pitches [i] : 0;
        if (!shares_lead (cxt, lead) || !staged_layouts (cxt, b->in, b->in_pitch, numInputFrames [i], b->out, b->out_pitch, numOutputFrames [i])) continue;
        if (!items && !(items = malloc (sizeof (ArtLayoutItem) * (size_t) n))) continue;       /* (no table: the single planar call stages itself) */
        const int C = cxt->numChannels;
        if (b->in_pitch) hip->d_in = arthip_grow (hip->d_in, &hip->in_cap, sizeof (art_s) * (size_t) numInputFrames [i] * C);
        if (b->out_pitch)                /* (room for the frames the call will make, not for the caller's whole capacity) */
            hip->d_out = arthip_grow (hip->d_out, &hip->out_cap,
                                      sizeof (art_s) * ((size_t) peek_call (cxt, numInputFrames [i], numOutputFrames [i], ratios [i]).output_generated + 16) * C);
        if ((b->in_pitch && !hip->d_in) || (b->out_pitch && !hip->d_out)) continue;            /* (... which then falls back as it always did) */
        b->staged = 1; ++staged;
        if (b->in_pitch) {
            ArtLayoutItem *it = &items [moved++];
            memset (it, 0, sizeof (*it));
            it->planes = (art_s *) b->in; it->frames = hip->d_in; it->pitch = b->in_pitch; it->count = numInputFrames [i]; it->C = C;
            b->in = hip->d_in; b->in_pitch = 0;
        }
        if (b->out_pitch) { b->out = hip->d_out; b->out_pitch = 0; }
    }
    if (batch_transpose (lead, items, moved, n, 0))
        for (int i = 0; i < n; ++i)
            if (io [i].staged) {
                io [i].in = d_inputs [i]; io [i].out = d_outputs [i]; io [i].staged = -1;
                io [i].in_pitch = in_pitches ? in_pitches [i] : 0; io [i].out_pitch = out_pitches ? out_pitches [i] : 0;
            }

    for (int i = 0; i < n; ++i) {
        const BatchIo *b = &io [i];
        /* (a flush handed to this phase is the single call) */
        const int how = numInputFrames [i] < 0 || b->staged < 0 ? 0 :
                        batch_plan (cxts [i], b->in, b->in_pitch, numInputFrames [i], b->out, b->out_pitch, numOutputFrames [i], ratios [i], lead->stream, NULL, &w);
        if (how == 1) { results [i] = w.plans [w.gathered].res; w.owner [w.gathered++] = i; }
        else if (how == 2) { results [i] = w.matrix_plans [w.matrix_gathered].res; w.matrix_owner [w.matrix_gathered++] = i; }
        else
            results [i] = device_call (cxts [i], b->in, b->in_pitch, numInputFrames [i], b->out, b->out_pitch, numOutputFrames [i], ratios [i]);
    }

    if (w.gathered) {
        /* the prefill fits of the first outputs, one launch in front of the FIR launches that read what they write */
        if (batch_launch (lead, &w)) {
            zero_results (results, w.owner, w.gathered);
            failed = -1;
        }
        else batch_commit (cxts, w.plans, w.owner, w.gathered, ART_KERNEL_GENERAL);
    }
    /* (the matrix-core calls are made whatever became of the general kernel's launch: other contexts) */
    rc = w.matrix_gathered ? batch_matrix (cxts, &w, io, numInputFrames, numOutputFrames, ratios, results) : 0;
    if (failed) rc = failed;

    /* the staged calls' outputs, back into the callers' planes */
    moved = 0;
    for (int i = 0; i < n && staged; ++i)
        if (io [i].staged > 0 && out_pitches && out_pitches [i] && results [i].output_generated) {
            ArtLayoutItem *it = &items [moved++];
            memset (it, 0, sizeof (*it));
            it->planes = d_outputs [i]; it->frames = cxts [i]->hip->d_out; it->pitch = out_pitches [i];
            it->count = (int) results [i].output_generated; it->C = cxts [i]->numChannels;
        }
    if (batch_transpose (lead, items, moved, n, 1)) rc = -1;
out:
    free (items);
    batch_work_free (&w);
    return rc;
}

/* both batch entries: the process phase, then (and_flush) the flushes */
static int batch_entry (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const long *in_pitches, const int *numInputFrames,
                        artsample_t *const *d_outputs, const long *out_pitches, const int *numOutputFrames, const double *ratios,
                        ResampleResult *results, int and_flush, int from_start);

int resampleProcessBatchInterleavedDevice (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const int *numInputFrames,
                                           artsample_t *const *d_outputs, const int *numOutputFrames, const double *ratios,
                                           ResampleResult *results)
{
    return batch_entry (cxts, n, d_inputs, NULL, numInputFrames, d_outputs, NULL, numOutputFrames, ratios, results, 0, 0);
}

int resampleProcessBatchPlanarDevice (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                      const int *numInputFrames, artsample_t *const *d_outputs, const long *outputPitches,
                                      const int *numOutputFrames, const double *ratios, ResampleResult *results)
{
    return batch_entry (cxts, n, d_inputs, inputPitches, numInputFrames, d_outputs, outputPitches, numOutputFrames, ratios, results, 0, 0);
}

/* ---- many whole clips, one launch per stage ------------------------------------------------------------------------
 * A clip is init / reset -> process -> flush, and the flush is the dear call of an EXTRAPOLATE_ENDPOINTS stream: one forward fit per
 * channel, each a one-wave workgroup that runs for milliseconds.  resampleProcessAndFlushBatchInterleavedDevice makes the batch's process
 * phase (above), then plans the flush of every context whose single resampleProcessAndFlushInterleavedDevice would go on to it, and
 * gathers them: all tail fits one launch (into one buffer of the lead's, a slice per context), the prefills of the streams whose first
 * output the flush makes a second, the flushes' FIR one more with their rolls.  Flushes that cannot be gathered are the single call. */
static int flush_due (const int *numInputFrames, const int *numOutputFrames, const ResampleResult *results, int i)
{
    /* (resampleProcessAndFlushInterleavedDevice's early return: input not all used, or no room left) */
    return numInputFrames [i] - (int) results [i].input_used == 0 && numOutputFrames [i] - (int) results [i].output_generated != 0;
}

static int batch_flush (Resample *const *cxts, int n, const long *in_pitches, const int *numInputFrames, artsample_t *const *d_outputs,
                        const long *out_pitches, const int *numOutputFrames, const double *ratios, ResampleResult *results)
{
    struct artamd_resampler *lead = cxts [0]->hip;
    BatchWork w;
    int rc = -1;

    size_t channels = 0, tail_samples = 0;
    for (int i = 0; i < n; ++i)
        if (flush_due (numInputFrames, numOutputFrames, results, i) && (cxts [i]->flags & EXTRAPOLATE_ENDPOINTS) && !cxts [i]->hip->nshards) {
            channels += (size_t) cxts [i]->numChannels;
            tail_samples += (size_t)(cxts [i]->numTaps / 2) * cxts [i]->numChannels;
        }
    if (batch_work_init (&w, n, channels, 0)) goto out;
    /* (no tails: the extrapolating contexts' flushes are made one by one) */
    if (tail_samples) lead->d_tails = arthip_grow (lead->d_tails, &lead->tails_cap, sizeof (art_s) * tail_samples);

    art_s *tail = lead->d_tails;
    for (int i = 0; i < n; ++i) {
        if (!flush_due (numInputFrames, numOutputFrames, results, i)) continue;
        Resample *cxt = cxts [i];
        const int cap = numOutputFrames [i] - (int) results [i].output_generated;
        /* (behind the process call's frames: in every plane, or in the interleaved buffer) */
        const long in_pitch = in_pitches ? in_pitches [i] : 0, out_pitch = out_pitches ? out_pitches [i] : 0;
        art_s *out = d_outputs [i] + (size_t) results [i].output_generated * (out_pitch ? 1 : cxt->numChannels);
        const int extrapolates = (cxt->flags & EXTRAPOLATE_ENDPOINTS) && !cxt->hip->nshards;

        if (batch_plan (cxt, NULL, 0, -1, out, out_pitch, cap, ratios [i], lead->stream, extrapolates ? tail : NULL, &w))
            w.owner [w.gathered++] = i;
        else
            results [i].output_generated += device_call (cxt, NULL, in_pitch, -1, out, out_pitch, cap, ratios [i]).output_generated;
        if (extrapolates && tail) tail += (size_t)(cxt->numTaps / 2) * cxt->numChannels;
    }

    if (w.gathered) {
        /* (a failed launch: the flushes of its contexts were not made — their results are the process phase's, as after a failed single flush) */
        if (batch_launch (lead, &w)) goto out;
        batch_commit (cxts, w.plans, w.owner, w.gathered, ART_KERNEL_GENERAL);
        for (int k = 0; k < w.gathered; ++k) results [w.owner [k]].output_generated += w.plans [k].res.output_generated;
    }
    rc = 0;
out:
    batch_work_free (&w);
    return rc;
}

/* resampleReset for every context of a list, on the lead's device: the contexts on the lead's stream and device that are not sharded share ONE
 * zeroing launch over both history buffers of each (so it is right whichever of the two is current), its table in the lead's batch table (the
 * batch launches that follow rewrite it in stream order); the others get their own resampleReset.  0, or -1 with no context reset. */
static int batch_from_start (Resample *const *cxts, int n)
{
    struct artamd_resampler *lead = cxts [0]->hip;
    ArtZeroRun *runs = malloc (sizeof (ArtZeroRun) * 2 * (size_t) n);
    int nruns = 0, rc = -1;
    if (!runs) goto out;
    for (int i = 0; i < n; ++i) {
        const struct artamd_resampler *hip = cxts [i]->hip;
        if (hip->nshards || hip->stream != lead->stream || hip->device != lead->device) continue;
        const long words = (long)(sizeof (art_s) / 4) * HIST_FRAMES (cxts [i]->numTaps) * cxts [i]->numChannels;
        for (int h = 0; h < 2; ++h) { runs [nruns].ptr = (unsigned int *) hip->d_hist [h]; runs [nruns].words = words; ++nruns; }
    }
    if (nruns) {
        const size_t need = sizeof (ArtZeroRun) * (size_t) nruns;
        if (need > lead->batch_cap) lead->d_batch = arthip_grow (lead->d_batch, &lead->batch_cap, need);
        if (!lead->d_batch || arthip_zero_runs (runs, nruns, lead->d_batch, lead->stream)) {
            fprintf (stderr, "artamd: resample clips: the zeroing launch failed: %s\n", arthip_last_error ());
            goto out;
        }
    }
    for (int i = 0; i < n; ++i) {
        const struct artamd_resampler *hip = cxts [i]->hip;
        if (hip->nshards || hip->stream != lead->stream || hip->device != lead->device) resampleReset (cxts [i]);
        else reset_host (cxts [i]);
    }
    rc = 0;
out:
    free (runs);
    return rc;
}

static int batch_entry (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const long *in_pitches, const int *numInputFrames,
                        artsample_t *const *d_outputs, const long *out_pitches, const int *numOutputFrames, const double *ratios,
                        ResampleResult *results, int and_flush, int from_start)
{
    if (n <= 0) return 0;
    if (artamd_batch_distinct ((const void *const *) cxts, n, stamp_of, "resample", "context")) return -1;
    struct artamd_resampler *lead = cxts [0]->hip;
    BatchIo *io = malloc (sizeof (BatchIo) * (size_t) n);
    ENTER_DEVICE (lead);
    if (io && from_start && batch_from_start (cxts, n)) {
        artamd_note_failure ("resampler: the clips entry could not put its contexts back (nothing enqueued)");
        LEAVE_DEVICE (lead);
        free (io);
        return -1;
    }
    int rc = io ? batch_process (cxts, n, d_inputs, in_pitches, numInputFrames, d_outputs, out_pitches, numOutputFrames, ratios, results, io) : -1;
    if (and_flush) {
        if (!rc) rc = batch_flush (cxts, n, in_pitches, numInputFrames, d_outputs, out_pitches, numOutputFrames, ratios, results);
        if (rc == -1) artamd_note_failure ("resampler: a launch of the batched process-and-flush failed");      /* (-2: counted where it failed) */
    }
    LEAVE_DEVICE (lead);
    free (io);
    return rc ? -1 : 0;
}

int resampleProcessAndFlushBatchInterleavedDevice (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const int *numInputFrames,
                                                   artsample_t *const *d_outputs, const int *numOutputFrames, const double *ratios,
                                                   ResampleResult *results)
{
    return batch_entry (cxts, n, d_inputs, NULL, numInputFrames, d_outputs, NULL, numOutputFrames, ratios, results, 1, 0);
}

int resampleProcessAndFlushBatchPlanarDevice (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                              const int *numInputFrames, artsample_t *const *d_outputs, const long *outputPitches,
                                              const int *numOutputFrames, const double *ratios, ResampleResult *results)
{
    return batch_entry (cxts, n, d_inputs, inputPitches, numInputFrames, d_outputs, outputPitches, numOutputFrames, ratios, results, 1, 0);
}

int resampleProcessAndFlushClipsPlanarDevice (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                              const int *numInputFrames, artsample_t *const *d_outputs, const long *outputPitches,
                                              const int *numOutputFrames, const double *ratios, int fromStart, ResampleResult *results)
{
    return batch_entry (cxts, n, d_inputs, inputPitches, numInputFrames, d_outputs, outputPitches, numOutputFrames, ratios, results, 1, fromStart != 0);
}

/* ---- the gradient of whole clips ---------------------------------------------------------------------------------------
 * resampleAdjointClipsPlanarDevice (art_hip.h): gx = A^T gy for the linear map A the clips entry applies from a fresh start.  The host's
 * part is the planner's: a clip's outputs are those of two calls replayed on a fresh POSITION (no context is touched) — the process
 * call of the clip's frames, then the flush's call of silence, each with all the room it can use.  Their segments go to the device as
 * they are; fir_adjoint.hip places every output with the forward's own locate (). */
typedef struct { ArtamdSegment *segs; int count, cap; } AdjointSegs;

/* one planned call appended to the list; returns its segment count, -1 out of memory */
static int adjoint_plan_call (ArtamdPosition *pos, int nIn, int cap, double ratio, ResampleResult *res, int *lin_floor, AdjointSegs *list)
{
    for (;;) {
        ArtamdPosition trial = *pos;
        const int nseg = artamdPlanCall (&trial, nIn, cap, ratio, res, list->segs + list->count, list->cap - list->count, lin_floor);
        if (nseg <= list->cap - list->count) { *pos = trial; list->count += nseg; return nseg; }
        ArtamdSegment *grown = realloc (list->segs, sizeof (ArtamdSegment) * ((size_t) list->count + nseg + 64));
        if (!grown) return -1;
        list->segs = grown; list->cap = list->count + nseg + 64;
    }
}

/* the clip of nIn frames a fresh context of cxt's parameters would make at `ratio`: both phases' outputs and segments; 0 or -1 */
static int adjoint_plan (const Resample *cxt, int nIn, double ratio, ArtAdjItem *it, AdjointSegs *list)
{
    ArtamdPosition pos;
    ResampleResult res;
    int lin_floor;

    /* (the position resampleReset leaves) */
    pos.numTaps = cxt->numTaps; pos.numFilters = cxt->numFilters; pos.flags = cxt->flags & ~(RESAMPLER_FLUSHED | EXTRAPOLATE_PREFILL);
    pos.inputIndex = cxt->numTaps; pos.floorActive = 0; pos.outputOffset = cxt->numTaps / 2; pos.fixedRatio = cxt->fixedRatio;

    memset (it, 0, sizeof (*it));
    it->seg_first [0] = list->count;
    if ((it->seg_count [0] = adjoint_plan_call (&pos, nIn, INT_MAX, ratio, &res, &lin_floor, list)) < 0) return -1;
    it->outputs [0] = res.output_generated;
    if ((int) res.input_used != nIn) return -1;        /* (cannot happen with that much room) */
    it->seg_first [1] = list->count;
    if ((it->seg_count [1] = adjoint_plan_call (&pos, -1, INT_MAX - (int) it->outputs [0], ratio, &res, &lin_floor, list)) < 0) return -1;
    it->outputs [1] = res.output_generated;
    it->lin_floor = lin_floor;

    it->bank = cxt->hip->d_bank;
    it->ratio = (cxt->flags & RESAMPLE_FIXED_RATIO) ? cxt->fixedRatio : ratio;
    it->in_frames = nIn; it->C = cxt->numChannels; it->T = cxt->numTaps; it->F = cxt->numFilters;
    it->interpolate = (cxt->flags & SUBSAMPLE_INTERPOLATE) != 0;
    it->lowpass = (cxt->flags & INCLUDE_LOWPASS) != 0;
    return 0;
}

int resampleAdjointClipsPlanarDevice (Resample *const *cxts, int n,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, const int *numOutputFrames,
        artsample_t *const *d_gradInputs, const long *gradInputPitches, const int *numInputFrames,
        const double *ratios)
{
    if (n <= 0) return 0;
    if (!cxts || !d_gradOutputs || !numOutputFrames || !d_gradInputs || !numInputFrames || !ratios) return -1;
    for (int i = 0; i < n; ++i) if (!cxts [i]) return -1;

    struct artamd_resampler *lead = cxts [0]->hip;
    for (int i = 0; i < n; ++i) {
        const struct artamd_resampler *hip = cxts [i]->hip;
        if (numInputFrames [i] < 0 || numOutputFrames [i] < 0) return -1;
        if (numInputFrames [i] > 0 && (!d_gradOutputs [i] || !d_gradInputs [i])) return -1;
        if ((cxts [i]->flags & EXTRAPOLATE_ENDPOINTS) || hip->nshards || hip->device != lead->device || hip->stream != lead->stream) return -1;
    }

    /* every item is planned (numOutputFrames [i] <= M_i is asked of an empty clip too); the empty ones are no items of the launches */
    ArtAdjItem *items = malloc (sizeof (ArtAdjItem) * (size_t) n);
    AdjointSegs list = { NULL, 0, 0 };
    int live = 0, rc = -1, refused = 0;
    if (!items) goto out;
    for (int i = 0; i < n; ++i) {
        ArtAdjItem *it = &items [live];
        const int kept = list.count;
        if (adjoint_plan (cxts [i], numInputFrames [i], ratios [i], it, &list)) goto out;
        if ((unsigned long) numOutputFrames [i] > (unsigned long) it->outputs [0] + it->outputs [1]) { refused = 1; goto out; }
        if (!numInputFrames [i]) { list.count = kept; continue; }
        it->gy = d_gradOutputs [i]; it->gy_pitch = gradOutputPitches ? gradOutputPitches [i] : 0; it->gy_frames = (unsigned int) numOutputFrames [i];
        it->gx = d_gradInputs [i]; it->gx_pitch = gradInputPitches ? gradInputPitches [i] : 0;
        ++live;
    }
    if (!live) { rc = 0; goto out; }

    {
        ENTER_DEVICE (lead);
        lead->d_batch = arthip_grow (lead->d_batch, &lead->batch_cap, arthip_fir_adjoint_bytes (live, list.count));
        rc = lead->d_batch ? arthip_fir_adjoint (items, live, list.segs, list.count, lead->d_batch, lead->stream) : -1;
        if (rc < 0) fprintf (stderr, "artamd: resample adjoint: launch failed: %s\n", arthip_last_error ());
        LEAVE_DEVICE (lead);
    }
out:
    if (rc < 0 && !refused) artamd_note_failure ("resampler: a launch of the clips adjoint failed");
    free (items);
    free (list.segs);
    return rc;
}

/* resampleAdjointScheduleClipsPlanarDevice (art_hip.h): the same for a clip made block by block — K process calls, each at its own ratio, then the
 * flush, replayed one after the other on ONE fresh position: K + 1 phases where the entry above has two.  Every replay keeps its own ratio,
 * segment slice, output count, first output among the clip's, the frames in front of it and its floor (ArtAdjPhase). */
typedef struct { ArtAdjPhase *phases; int count, cap; } AdjointPhases;

static ArtAdjPhase *adjoint_phase_new (AdjointPhases *list)
{
    if (list->count == list->cap) {
        ArtAdjPhase *grown = realloc (list->phases, sizeof (ArtAdjPhase) * ((size_t) list->cap * 2 + 64));
        if (!grown) return NULL;
        list->phases = grown; list->cap = list->cap * 2 + 64;
    }
    ArtAdjPhase *ph = &list->phases [list->count++];
    memset (ph, 0, sizeof (*ph));
    return ph;
}

/* the clip a fresh context of cxt's parameters would make of the blocks; 0, -1 out of memory, -2 a clip the entry refuses (a ratio no call
 * can be made at, more outputs than an int counts) */
static int adjoint_plan_blocks (const Resample *cxt, int numBlocks, const int *frames, const double *ratios, ArtAdjBlocksItem *it,
                                unsigned long *outputs, AdjointPhases *phases, AdjointSegs *list)
{
    ArtamdPosition pos;
    ResampleResult res;
    int lin_floor, before = 0;
    unsigned long made = 0;
    const int fixed = (cxt->flags & RESAMPLE_FIXED_RATIO) != 0;
    double ratio = cxt->fixedRatio;

    /* (the position resampleReset leaves) */
    pos.numTaps = cxt->numTaps; pos.numFilters = cxt->numFilters; pos.flags = cxt->flags & ~(RESAMPLER_FLUSHED | EXTRAPOLATE_PREFILL);
    pos.inputIndex = cxt->numTaps; pos.floorActive = 0; pos.outputOffset = cxt->numTaps / 2; pos.fixedRatio = cxt->fixedRatio;

    memset (it, 0, sizeof (*it));
    it->phase_first = phases->count;
    for (int k = 0; k <= numBlocks; ++k) {                 /* (k == numBlocks: the flush's call of silence, at the last block's ratio) */
        const int flush = k == numBlocks, nIn = flush ? -1 : frames [k];
        ArtAdjPhase *ph = adjoint_phase_new (phases);
        if (!ph) return -1;
        if (!flush && !fixed) ratio = ratios [k];
        if (made > (unsigned long) INT_MAX) return -2;
        ph->seg_first = list->count;
        if ((ph->seg_count = adjoint_plan_call (&pos, nIn, flush ? INT_MAX - (int) made : INT_MAX, ratio, &res, &lin_floor, list)) < 0) return -1;
        if (!flush && (int) res.input_used != nIn) return -2;          /* (with that much room: a ratio that is not > 0) */
        ph->ratio = ratio;
        ph->outputs = res.output_generated; ph->first_output = (unsigned int) made;
        ph->start = before; ph->end = flush ? before : before + nIn;
        ph->floor = lin_floor > 0 ? lin_floor : 0;
        made += res.output_generated;
        if (!flush) before += nIn;
    }
    if (made > (unsigned long) INT_MAX) return -2;
    it->phase_count = numBlocks + 1;
    *outputs = made;

    it->bank = cxt->hip->d_bank;
    it->in_frames = before; it->C = cxt->numChannels; it->T = cxt->numTaps; it->F = cxt->numFilters;
    it->interpolate = (cxt->flags & SUBSAMPLE_INTERPOLATE) != 0;
    it->lowpass = (cxt->flags & INCLUDE_LOWPASS) != 0;
    return 0;
}

/* The contexts no entry that only reads them takes (the gradient entries of such clips, and the sampling entries further down): 1 for a NULL
 * context, a context with EXTRAPOLATE_ENDPOINTS, a sharded one, one on another device or stream than cxts [0]. */
static int clip_contexts_refused (Resample *const *cxts, int n)
{
    for (int i = 0; i < n; ++i) if (!cxts [i]) return 1;

    const struct artamd_resampler *lead = cxts [0]->hip;
    for (int i = 0; i < n; ++i) {
        const struct artamd_resampler *hip = cxts [i]->hip;
        if ((cxts [i]->flags & EXTRAPOLATE_ENDPOINTS) || hip->nshards || hip->device != lead->device || hip->stream != lead->stream) return 1;
    }
    return 0;
}

/* What both gradient entries of such clips refuse before anything is planned, the same way: 1 for the contexts above, and per item with blocks
 * a NULL block array, a negative
 * count, more than INT_MAX frames, or a NULL buffer (`one` [i], `other` [i]: the entry's two sample buffers) where the clip has frames. */
static int clip_blocks_refused (Resample *const *cxts, int n, const int *numBlocks, const int *numOutputFrames, const int *const *numInputFrames,
                                const double *const *ratios, const void *const *one, const void *const *other)
{
    if (clip_contexts_refused (cxts, n)) return 1;

    for (int i = 0; i < n; ++i) {
        if (numBlocks [i] <= 0) continue;
        if (!numInputFrames [i] || numOutputFrames [i] < 0) return 1;
        if (!ratios [i] && !(cxts [i]->flags & RESAMPLE_FIXED_RATIO)) return 1;
        long frames = 0;
        for (int k = 0; k < numBlocks [i]; ++k) {
            if (numInputFrames [i] [k] < 0) return 1;
            if ((frames += numInputFrames [i] [k]) > INT_MAX) return 1;
        }
        if (frames > 0 && (!one [i] || !other [i])) return 1;
    }
    return 0;
}

/* The phase replay of both entries: every item with blocks is planned (numOutputFrames [i] <= M_i is asked of an empty clip too) into items
 * [0, live), `which` [q] the call's index of item q; an empty clip is an item only where keep_empty.  Returns live, or -1 (out of memory) or -2
 * (refused: a clip adjoint_plan_blocks refuses, numOutputFrames [i] > M_i). */
static int clip_blocks_plan (Resample *const *cxts, int n, const int *numBlocks, const int *numOutputFrames, const int *const *numInputFrames,
                             const double *const *ratios, int keep_empty, ArtAdjBlocksItem *items, int *which, AdjointPhases *phases, AdjointSegs *list)
{
    int live = 0;
    for (int i = 0; i < n; ++i) {
        if (numBlocks [i] <= 0) continue;
        ArtAdjBlocksItem *it = &items [live];
        const int kept = list->count, kept_phases = phases->count;
        unsigned long outputs = 0;
        const int planned = adjoint_plan_blocks (cxts [i], numBlocks [i], numInputFrames [i], ratios [i], it, &outputs, phases, list);
        if (planned) return planned;
        if ((unsigned long) numOutputFrames [i] > outputs) return -2;
        if (!it->in_frames && !keep_empty) { list->count = kept; phases->count = kept_phases; continue; }
        which [live++] = i;
    }
    return live;
}

int resampleAdjointScheduleClipsPlanarDevice (Resample *const *cxts, int n, const int *numBlocks,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, const int *numOutputFrames,
        artsample_t *const *d_gradInputs, const long *gradInputPitches,
        const int *const *numInputFrames, const double *const *ratios)
{
    if (n <= 0) return 0;
    if (!cxts || !numBlocks || !d_gradOutputs || !numOutputFrames || !d_gradInputs || !numInputFrames || !ratios) return -1;
    if (clip_blocks_refused (cxts, n, numBlocks, numOutputFrames, numInputFrames, ratios, (const void *const *) d_gradOutputs, (const void *const *) d_gradInputs))
        return -1;

    /* the empty clips are no items of the launches */
    struct artamd_resampler *lead = cxts [0]->hip;
    ArtAdjBlocksItem *items = malloc (sizeof (ArtAdjBlocksItem) * (size_t) n);
    int *which = malloc (sizeof (int) * (size_t) n);
    AdjointSegs list = { NULL, 0, 0 };
    AdjointPhases phases = { NULL, 0, 0 };
    int live = 0, rc = -1, refused = 0;
    if (!items || !which) goto out;
    live = clip_blocks_plan (cxts, n, numBlocks, numOutputFrames, numInputFrames, ratios, 0, items, which, &phases, &list);
    if (live < 0) { refused = live == -2; goto out; }
    for (int q = 0; q < live; ++q) {
        ArtAdjBlocksItem *it = &items [q];
        const int i = which [q];
        it->gy = d_gradOutputs [i]; it->gy_pitch = gradOutputPitches ? gradOutputPitches [i] : 0; it->gy_frames = (unsigned int) numOutputFrames [i];
        it->gx = d_gradInputs [i]; it->gx_pitch = gradInputPitches ? gradInputPitches [i] : 0;
    }
    if (!live) { rc = 0; goto out; }

    {
        ENTER_DEVICE (lead);
        lead->d_batch = arthip_grow (lead->d_batch, &lead->batch_cap, arthip_fir_adjoint_blocks_bytes (live, phases.count, list.count));
        rc = lead->d_batch ? arthip_fir_adjoint_blocks (items, live, phases.phases, phases.count, list.segs, list.count, lead->d_batch, lead->stream) : -1;
        if (rc < 0) fprintf (stderr, "artamd: resample schedule adjoint: launch failed: %s\n", arthip_last_error ());
        LEAVE_DEVICE (lead);
    }
out:
    if (rc < 0 && !refused) artamd_note_failure ("resampler: a launch of the schedule clips adjoint failed");
    free (items);
    free (which);
    free (phases.phases);
    free (list.segs);
    return rc;
}

/* resampleRateGradientScheduleClipsPlanarDevice (art_hip.h): the gradient of the same clips with respect to their blocks' ratios, from the same
 * phase replay; fir_rate_grad.hip reads the samples where the adjoint writes their gradient.  An empty clip is an item too (its block gets
 * a zero), with no gradient frames to read. */
int resampleRateGradientScheduleClipsPlanarDevice (Resample *const *cxts, int n, const int *numBlocks,
        const artsample_t *const *d_inputs, const long *inputPitches,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, const int *numOutputFrames,
        const int *const *numInputFrames, const double *const *ratios,
        double *const *d_gradRatios)
{
    if (n <= 0) return 0;
    if (!cxts || !numBlocks || !d_inputs || !d_gradOutputs || !numOutputFrames || !numInputFrames || !ratios || !d_gradRatios) return -1;
    if (clip_blocks_refused (cxts, n, numBlocks, numOutputFrames, numInputFrames, ratios, (const void *const *) d_gradOutputs, (const void *const *) d_inputs))
        return -1;
    for (int i = 0; i < n; ++i) {
        /* (without interpolation an output does not move with the ratio until it changes rows: a gradient of zero almost everywhere; a
         * fixed-ratio context ignores the ratios it would be the gradient of) */
        if (!(cxts [i]->flags & SUBSAMPLE_INTERPOLATE) || (cxts [i]->flags & RESAMPLE_FIXED_RATIO)) return -1;
        if (numBlocks [i] > 0 && !d_gradRatios [i]) return -1;
    }

    struct artamd_resampler *lead = cxts [0]->hip;
    ArtAdjBlocksItem *planned = malloc (sizeof (ArtAdjBlocksItem) * (size_t) n);
    ArtRateItem *items = malloc (sizeof (ArtRateItem) * (size_t) n);
    int *which = malloc (sizeof (int) * (size_t) n);
    AdjointSegs list = { NULL, 0, 0 };
    AdjointPhases phases = { NULL, 0, 0 };
    int live = 0, rc = -1, refused = 0;
    if (!planned || !items || !which) goto out;
    live = clip_blocks_plan (cxts, n, numBlocks, numOutputFrames, numInputFrames, ratios, 1, planned, which, &phases, &list);
    if (live < 0) { refused = live == -2; goto out; }
    if (arthip_fir_rate_grad_tiles (phases.phases, phases.count) > (unsigned long) INT_MAX) { refused = 1; goto out; }
    for (int q = 0; q < live; ++q) {
        const ArtAdjBlocksItem *from = &planned [q];
        ArtRateItem *it = &items [q];
        const int i = which [q];
        memset (it, 0, sizeof (*it));
        it->bank = from->bank; it->in_frames = from->in_frames; it->C = from->C; it->T = from->T; it->F = from->F;
        it->phase_first = from->phase_first; it->phase_count = from->phase_count;
        it->x = d_inputs [i]; it->x_pitch = inputPitches ? inputPitches [i] : 0;
        it->gy = d_gradOutputs [i]; it->gy_pitch = gradOutputPitches ? gradOutputPitches [i] : 0;
        it->gy_frames = from->in_frames ? (unsigned int) numOutputFrames [i] : 0;
        it->grad = d_gradRatios [i];
    }
    if (!live) { rc = 0; goto out; }

    {
        ENTER_DEVICE (lead);
        lead->d_batch = arthip_grow (lead->d_batch, &lead->batch_cap,
                                     arthip_fir_rate_grad_bytes (live, phases.count, list.count, arthip_fir_rate_grad_tiles (phases.phases, phases.count)));
        rc = lead->d_batch ? arthip_fir_rate_grad (items, live, phases.phases, phases.count, list.segs, list.count, lead->d_batch, lead->stream) : -1;
        if (rc < 0) fprintf (stderr, "artamd: resample rate gradient: launch failed: %s\n", arthip_last_error ());
        LEAVE_DEVICE (lead);
    }
out:
    if (rc < 0 && !refused) artamd_note_failure ("resampler: a launch of the schedule clips rate gradient failed");
    free (planned);
    free (items);
    free (which);
    free (phases.phases);
    free (list.segs);
    return rc;
}

/* ---- whole clips at a position curve in device memory ------------------------------------------------------------------
 * resampleSampleClipsPlanarDevice, resampleSampleAdjointClipsPlanarDevice, resampleSamplePositionGradientClipsPlanarDevice and, on a LADDER of
 * banks with a level per output, resampleSampleBandClipsPlanarDevice, resampleSampleBandAdjointClipsPlanarDevice,
 * resampleSampleBandGradientsClipsPlanarDevice (art_hip.h): no planner and no context state — a context supplies its bank and flags, every
 * output's position comes from the caller's curve, and fir_sample.hip does the rest in one launch.  The six entries are one function: `what`
 * says which buffers an item needs (d_in: x; d_gy; d_out: y or gx; d_gp, d_gl) and when it is part of the launch, `band` which family
 * calls; the unbanded three bring numRungs = 0 and no d_levels, one context per clip.  On the banded three rung k of clip i is
 * cxts [i * numRungs + k], the levels lie beside the positions, the per-clip checks are made on rung 0 with the ladder's on top, and the
 * gradients entry takes d_gp, d_gl or both. */
static int sample_entry (int what, int band, const char *name, Resample *const *cxts, int n, int numRungs,
                         const art_s *const *d_in, const long *inPitches, const int *numInputFrames,
                         const double *const *d_positions, const double *const *d_levels, const int *numOutputFrames,
                         const art_s *const *d_gy, const long *gyPitches, art_s *const *d_out, const long *outPitches,
                         double *const *d_gp, double *const *d_gl)
{
    const int reads_in = what != ART_SAMPLE_ADJOINT, reads_gy = what != ART_SAMPLE_FORWARD, writes_out = what != ART_SAMPLE_SLOPE;
    const int rungs = band ? numRungs : 1;

    if (n <= 0) return 0;
    if (band && (numRungs < 1 || numRungs > ART_BAND_RUNGS || n > INT_MAX / ART_BAND_RUNGS)) return -1;
    if (!cxts || !numInputFrames || !d_positions || (band && !d_levels) || !numOutputFrames || (reads_in && !d_in) || (reads_gy && !d_gy) ||
        (writes_out && !d_out) || (!writes_out && !d_gp && !d_gl)) return -1;
    if (clip_contexts_refused (cxts, n * rungs)) return -1;
    for (int i = 0; i < n; ++i) {
        const Resample *lead = cxts [i * rungs];
        const int nIn = numInputFrames [i], nOut = numOutputFrames [i];
        for (int k = 0; band && k < rungs; ++k) {
            const Resample *rung = cxts [i * rungs + k];
            if (rung->numChannels != lead->numChannels || rung->numTaps != lead->numTaps || rung->numFilters != lead->numFilters) return -1;
            /* (two rungs are blended value by value of one interpolation cell: both interpolate) */
            if (!(rung->flags & SUBSAMPLE_INTERPOLATE)) return -1;
        }
        if (nIn < 0 || nOut < 0 || nIn > INT_MAX - 2 * lead->numTaps) return -1;
        /* (the slope of a nearest-filter context is zero almost everywhere) */
        if (what == ART_SAMPLE_SLOPE && !(lead->flags & SUBSAMPLE_INTERPOLATE)) return -1;
        if (!nOut || (what == ART_SAMPLE_ADJOINT && !nIn)) continue;
        if (!d_positions [i] || (band && !d_levels [i]) || (reads_in && nIn && !d_in [i]) || (reads_gy && !d_gy [i]) || (writes_out && !d_out [i]) ||
            (d_gp && !d_gp [i]) || (d_gl && !d_gl [i])) return -1;
    }

    struct artamd_resampler *lead = cxts [0]->hip;
    ArtSampleItem *items = malloc (sizeof (ArtSampleItem) * (size_t) n);
    unsigned long tasks = 0;
    int live = 0, rc = -1, refused = 0;
    if (!items) goto out;
    for (int i = 0; i < n; ++i) {
        const Resample *cxt = cxts [i * rungs];
        ArtSampleItem *it = &items [live];
        if (!numOutputFrames [i] || (what == ART_SAMPLE_ADJOINT && !numInputFrames [i])) continue;     /* (no task: no item) */
        memset (it, 0, sizeof (*it));
        for (int k = 0; k < rungs; ++k) it->bank [k] = cxts [i * rungs + k]->hip->d_bank;
        it->rungs = rungs;
        it->pos = d_positions [i]; it->level = band ? d_levels [i] : NULL;
        it->gy_frames = (unsigned int) numOutputFrames [i]; it->in_frames = numInputFrames [i];
        it->C = cxt->numChannels; it->T = cxt->numTaps; it->F = cxt->numFilters;
        it->interpolate = (cxt->flags & SUBSAMPLE_INTERPOLATE) != 0;
        it->lowpass = (cxt->flags & INCLUDE_LOWPASS) != 0;
        if (reads_in) { it->in = d_in [i]; it->in_pitch = inPitches ? inPitches [i] : 0; }
        if (reads_gy) { it->gy = d_gy [i]; it->gy_pitch = gyPitches ? gyPitches [i] : 0; }
        if (writes_out) { it->out = d_out [i]; it->out_pitch = outPitches ? outPitches [i] : 0; }
        else { it->gp = d_gp ? d_gp [i] : NULL; it->gl = d_gl ? d_gl [i] : NULL; }
        tasks += arthip_fir_sample_tasks (it, what);
        ++live;
    }
    if (tasks > (unsigned long) INT_MAX) { refused = 1; goto out; }
    if (!live) { rc = 0; goto out; }

    {
        ENTER_DEVICE (lead);
        lead->d_batch = arthip_grow (lead->d_batch, &lead->batch_cap, arthip_fir_sample_bytes (live));
        rc = lead->d_batch ? arthip_fir_sample (items, live, what, band, lead->d_batch, lead->stream) : -1;
        if (rc < 0) fprintf (stderr, "artamd: %s: launch failed: %s\n", name, arthip_last_error ());
        LEAVE_DEVICE (lead);
    }
out:
    if (rc < 0 && !refused)
        artamd_note_failure (band ? "resampler: a launch of the banded clips sampler failed" : "resampler: a launch of the clips sampler failed");
    free (items);
    return rc;
}

int resampleSampleClipsPlanarDevice (Resample *const *cxts, int n,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames,
        const double *const *d_positions, const int *numOutputFrames,
        artsample_t *const *d_outputs, const long *outputPitches)
{
    return sample_entry (ART_SAMPLE_FORWARD, 0, "resample sample", cxts, n, 0, d_inputs, inputPitches, numInputFrames, d_positions, NULL, numOutputFrames,
                         NULL, NULL, d_outputs, outputPitches, NULL, NULL);
}

int resampleSampleAdjointClipsPlanarDevice (Resample *const *cxts, int n,
        const double *const *d_positions, const int *numOutputFrames,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches,
        artsample_t *const *d_gradInputs, const long *gradInputPitches, const int *numInputFrames)
{
    return sample_entry (ART_SAMPLE_ADJOINT, 0, "resample sample adjoint", cxts, n, 0, NULL, NULL, numInputFrames, d_positions, NULL, numOutputFrames,
                         d_gradOutputs, gradOutputPitches, d_gradInputs, gradInputPitches, NULL, NULL);
}

int resampleSamplePositionGradientClipsPlanarDevice (Resample *const *cxts, int n,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames,
        const double *const *d_positions, const int *numOutputFrames,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches,
        double *const *d_gradPositions)
{
    return sample_entry (ART_SAMPLE_SLOPE, 0, "resample sample position gradient", cxts, n, 0, d_inputs, inputPitches, numInputFrames, d_positions, NULL,
                         numOutputFrames, d_gradOutputs, gradOutputPitches, NULL, NULL, d_gradPositions, NULL);
}

int resampleSampleBandClipsPlanarDevice (Resample *const *cxts, int n, int numRungs,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames,
        const double *const *d_positions, const double *const *d_levels, const int *numOutputFrames,
        artsample_t *const *d_outputs, const long *outputPitches)
{
    return sample_entry (ART_SAMPLE_FORWARD, 1, "resample sample band", cxts, n, numRungs, d_inputs, inputPitches, numInputFrames, d_positions, d_levels,
                         numOutputFrames, NULL, NULL, d_outputs, outputPitches, NULL, NULL);
}

int resampleSampleBandAdjointClipsPlanarDevice (Resample *const *cxts, int n, int numRungs,
        const double *const *d_positions, const double *const *d_levels, const int *numOutputFrames,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches,
        artsample_t *const *d_gradInputs, const long *gradInputPitches, const int *numInputFrames)
{
    return sample_entry (ART_SAMPLE_ADJOINT, 1, "resample sample band adjoint", cxts, n, numRungs, NULL, NULL, numInputFrames, d_positions, d_levels,
                         numOutputFrames, d_gradOutputs, gradOutputPitches, d_gradInputs, gradInputPitches, NULL, NULL);
}

int resampleSampleBandGradientsClipsPlanarDevice (Resample *const *cxts, int n, int numRungs,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames,
        const double *const *d_positions, const double *const *d_levels, const int *numOutputFrames,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches,
        double *const *d_gradPositions, double *const *d_gradLevels)
{
    return sample_entry (ART_SAMPLE_SLOPE, 1, "resample sample band gradients", cxts, n, numRungs, d_inputs, inputPitches, numInputFrames, d_positions,
                         d_levels, numOutputFrames, d_gradOutputs, gradOutputPitches, NULL, NULL, d_gradPositions, d_gradLevels);
}

/* ---- consecutive blocks of one stream, one launch --------------------------------------------------------------------
 * An ASRC loop makes a call per block with that block's ratio; each call is a launch with its own planning, staging and launch floor.
 * Where the caller knows the next blocks' ratios, resampleProcessScheduleInterleavedDevice plans them one after the other on the context
 * exactly as the single calls would, GATHERS those the single call would give to the general kernel into runs — one launch each
 * (fir_general_schedule_kernel) and one history roll, riding along — and makes every other block (a flush, a block for the matrix-core
 * path, a context the batch would not gather either) as its single call, behind the run before it.  A gathered block's position is
 * committed as it is planned; its history only by its run's launch. */
#define RUN_FRAMES_MAX (INT_MAX / 4)       /* input frames of one run: its linear indices (history ++ input) stay ints */

typedef struct {
    const art_s *in; art_s *out;         /* the run's first input / output frame */
    long in_pitch, out_pitch;            /* samples between their planes (0: interleaved frames) */
    int gathered, first;                 /* blocks in the run (outputs or not), the index of its first in `results` */
    int frames; unsigned int outputs;    /* its input frames (appended to the history by its launch) and output frames */
    ArtamdPosition start;                /* the context's position before the run */
    ArtSchedBlock *blocks; int *floors; int nblocks, block_cap;     /* the blocks with outputs; their own lin_floor */
    ArtSchedSeg *segs; int nsegs, seg_cap;
} SchedRun;

/* Plan block `k` as the single call would; gather it into the run if the general kernel is the single call's (1), else leave the context
 * as it stands (0) */
static int sched_gather (Resample *cxt, SchedRun *run, const art_s *in, long in_pitch, int nIn, art_s *out, long out_pitch, int cap, double ratio,
                         ResampleResult *res, int k)
{
    struct artamd_resampler *hip = cxt->hip;
    CallPlan p;
    ArtFirArgs a;
    ArtSegTable tab;

    if (!gatherable (cxt, 0, 0)) return 0;
    const int nseg = plan_one_call (cxt, nIn, cap, ratio, &p);
    const int lin_floor = p.lin_floor;
    if (nseg < 0) return 0;                                              /* (out of memory: the single call reports it) */
    *res = p.res;
    if (res->output_generated) {
        plan_args (cxt, &p, ratio, in, in_pitch, out, out_pitch, NULL, &a, &tab);
        a.lin_origin = hip->lin_origin + run->frames;                    /* (the run's earlier blocks are not in the history yet) */
        keep_rows (hip, &a);
        /* (the matrix-core path takes interleaved frames only: a block in planes goes where the interleaved schedule's would — its single call stages for it) */
        ArtFirArgs frames = a;
        frames.in_pitch = frames.out_pitch = 0;
        if (!general_call (cxt, &frames, &tab, res->output_generated) || !arthip_fir_schedule_accepts (&a, hip->segs, nseg, res->output_generated)) return 0;
        if (run->nblocks == run->block_cap) {
            const int want = run->block_cap ? 2 * run->block_cap : 16;
            ArtSchedBlock *b = realloc (run->blocks, sizeof (ArtSchedBlock) * (size_t) want);
            if (b) run->blocks = b;
            int *f = realloc (run->floors, sizeof (int) * (size_t) want);
            if (f) run->floors = f;
            if (!b || !f) return 0;
            run->block_cap = want;
        }
        if (run->nsegs + nseg > run->seg_cap) {
            const int want = 2 * (run->nsegs + nseg) + 64;
            ArtSchedSeg *g = realloc (run->segs, sizeof (ArtSchedSeg) * (size_t) want);
            if (!g) return 0;
            run->segs = g; run->seg_cap = want;
        }
        ArtSchedBlock *b = &run->blocks [run->nblocks];
        memset (b, 0, sizeof (*b));
        b->ratio = a.ratio;
        b->out_off = run->outputs; b->outputs = res->output_generated;
        b->in_off = run->frames; b->in_end = run->frames + (int) res->input_used;
        b->lin_floor = run->frames + (lin_floor > 0 ? lin_floor : 0);      /* (load_frame: below the floor, or below 0) */
        b->seg_begin = run->nsegs; b->seg_end = run->nsegs + nseg;
        for (int q = 0; q < nseg; ++q) {
            ArtSchedSeg *g = &run->segs [run->nsegs + q];
            g->first = hip->segs [q].first_output; g->lin_base = hip->segs [q].lin_base; g->base = hip->segs [q].base_offset;
        }
        run->floors [run->nblocks++] = lin_floor;
        run->nsegs += nseg;
    }
    if (!run->gathered++) { run->in = in; run->out = out; run->in_pitch = in_pitch; run->out_pitch = out_pitch; run->first = k; run->start = position_of (cxt); }
    hip->last_gathered = 1;
    run->frames += (int) res->input_used; run->outputs += res->output_generated;
    commit_position (cxt, &p.trial, res->output_generated != 0);
    return 1;
}

/* The pending run's launch arguments (nblocks > 0) — and, on the way, the upkeep of the kept rows, block by block, with the arguments and
 * tables of the single call's launches */
static void sched_run_args (Resample *cxt, const SchedRun *run, ArtFirArgs *a)
{
    struct artamd_resampler *hip = cxt->hip;
    const int C = cxt->numChannels;
    ArtSegTable tab;
    for (int i = 0; i < run->nblocks; ++i) {
        const ArtSchedBlock *b = &run->blocks [i];
        fill_args (cxt, a, b->ratio, run->in + (size_t) b->in_off * (run->in_pitch ? 1 : C), run->in_pitch, b->in_end - b->in_off,
                   run->out + (size_t) b->out_off * (run->out_pitch ? 1 : C), run->out_pitch);
        a->lin_origin = hip->lin_origin + b->in_off;
        keep_rows (hip, a);
        if (!a->rows_cache) continue;
        const int nseg = b->seg_end - b->seg_begin;
        for (int s0 = 0; s0 < nseg; s0 += ART_MAX_SEGS) {
            const int s1 = s0 + ART_MAX_SEGS < nseg ? s0 + ART_MAX_SEGS : nseg;
            tab.count = s1 - s0; tab.lin_floor = run->floors [i];
            for (int q = s0; q < s1; ++q) {
                const ArtSchedSeg *g = &run->segs [b->seg_begin + q];
                tab.first [q - s0] = g->first; tab.lin_base [q - s0] = g->lin_base; tab.base [q - s0] = g->base;
            }
            a->n_begin = run->segs [b->seg_begin + s0].first;
            a->n_end = s1 < nseg ? run->segs [b->seg_begin + s1].first : b->outputs;
            if (a->n_end > a->n_begin) arthip_fir_rows_touch (a, &tab);
        }
    }
    fill_args (cxt, a, run->blocks [0].ratio, run->in, run->in_pitch, run->frames, run->out, run->out_pitch);
    a->roll_dst = run->frames > 0 ? hip->d_hist [hip->cur ^ 1] : NULL;
    a->roll_appended = run->frames;
}

static void sched_run_clear (SchedRun *run)
{
    run->gathered = run->nblocks = run->nsegs = run->frames = 0; run->outputs = 0;
}

/* the run's launch failed, or was never made: the context is back where it stood before the run, the run's results are { 0, 0 } */
static void sched_run_undo (Resample *cxt, SchedRun *run, ResampleResult *results)
{
    cxt->outputOffset = run->start.outputOffset; cxt->inputIndex = run->start.inputIndex;
    cxt->flags = run->start.flags; cxt->hip->floor_active = run->start.floorActive;
    zero_results (results + run->first, NULL, run->gathered);
    sched_run_clear (run);
}

/* the run's launch (if it has blocks: `launched`) is on the stream: the history behind it, rolled here unless the launch took the roll along */
static void sched_run_done (Resample *cxt, SchedRun *run, int launched, int rolled)
{
    struct artamd_resampler *hip = cxt->hip;
    if (launched) { hip->last_kernel = ART_KERNEL_GENERAL; hip->last_fixed [0] = 0; }
    if (run->frames > 0 && !rolled)
        arthip_roll_history (hip->d_hist [hip->cur ^ 1], hip->d_hist [hip->cur], run->in, run->in_pitch, run->frames, HIST_FRAMES (cxt->numTaps), cxt->numChannels, hip->stream);
    commit_history (hip, run->frames);
    sched_run_clear (run);
}

/* Launch the pending run and roll the history behind it.  -1: the launch failed — nothing of it was enqueued, the context is back where it
 * stood before the run and the run's results are { 0, 0 } */
static int sched_launch (Resample *cxt, SchedRun *run, ResampleResult *results)
{
    struct artamd_resampler *hip = cxt->hip;
    int rolled = 0;

    if (!run->gathered) return 0;
    if (run->nblocks) {
        ArtFirArgs a;
        sched_run_args (cxt, run, &a);
        take_events (hip, &a);
        hip->d_sched = arthip_grow (hip->d_sched, &hip->sched_cap, arthip_fir_schedule_bytes (run->nblocks, run->nsegs));
        const int k = hip->d_sched ? arthip_fir_schedule (&a, run->blocks, run->nblocks, run->segs, run->nsegs, hip->d_sched, hip->stream) : -1;
        if (k < 0) {
            return_events (hip);
            artamd_note_failure ("resampler: schedule launch failed");
            sched_run_undo (cxt, run, results);
            return -1;
        }
        rolled = (k & ART_FIR_ROLLED) != 0;
    }
    sched_run_done (cxt, run, run->nblocks != 0, rolled);
    return 0;
}

/* a block's buffers: `frames` frames into the interleaved buffer, or into every plane */
static const art_s *sched_at (const art_s *base, long pitch, size_t frames, int C) { return base ? base + frames * (pitch ? 1 : (size_t) C) : NULL; }

/* a block as its single call, in the layout of the schedule's buffers */
static ResampleResult sched_single (Resample *cxt, const art_s *in, long in_pitch, int nIn, art_s *out, long out_pitch, int cap, double ratio, int flush)
{
    if (!in_pitch && !out_pitch)
        return flush ? resampleProcessAndFlushInterleavedDevice (cxt, in, nIn, out, cap, ratio) : resampleProcessInterleavedDevice (cxt, in, nIn, out, cap, ratio);
    return flush ? resampleProcessAndFlushPlanarDevice (cxt, in, in_pitch, nIn, out, out_pitch, cap, ratio)
                 : resampleProcessPlanarDevice (cxt, in, in_pitch, nIn, out, out_pitch, cap, ratio);
}

/* one stream's schedule (numBlocks > 0, no negative frame count): *made = the blocks made; 0, or -1: a launch failed */
static int schedule_one (Resample *cxt, int numBlocks, const art_s *d_input, long in_pitch, const int *numInputFrames, art_s *d_output, long out_pitch,
                         const int *numOutputFrames, const double *ratios, int flushLast, ResampleResult *results, int *made_out)
{
    zero_results (results, NULL, numBlocks);
    struct artamd_resampler *hip = cxt->hip;
    const int C = cxt->numChannels;
    SchedRun run;
    memset (&run, 0, sizeof (run));
    size_t in_pos = 0, out_pos = 0;
    int made = 0, failed = 0;

    ENTER_DEVICE (hip);
    for (int k = 0; k < numBlocks && !failed; ++k) {
        const art_s *in = sched_at (d_input, in_pitch, in_pos, C);
        art_s *out = (art_s *) sched_at (d_output, out_pitch, out_pos, C);
        const int flush = flushLast && k == numBlocks - 1;
        if (run.gathered && run.frames > RUN_FRAMES_MAX - numInputFrames [k] && sched_launch (cxt, &run, results)) { failed = 1; break; }
        if (flush || !sched_gather (cxt, &run, in, in_pitch, numInputFrames [k], out, out_pitch, numOutputFrames [k], ratios [k], &results [k], k)) {
            /* the single call, behind the run before it (a failure of its own: { 0, 0 } and the count in artamdErrorCount) */
            if (sched_launch (cxt, &run, results)) { failed = 1; break; }
            const int errors = artamdErrorCount ();
            results [k] = sched_single (cxt, in, in_pitch, numInputFrames [k], out, out_pitch, numOutputFrames [k], ratios [k], flush);
            if (artamdErrorCount () != errors) { zero_results (&results [k], NULL, 1); failed = 1; break; }
        }
        made = k + 1;
        if ((int) results [k].input_used != numInputFrames [k]) break;          /* a cap too small: no later block is made */
        in_pos += (size_t) numInputFrames [k]; out_pos += results [k].output_generated;
    }
    if (!failed && sched_launch (cxt, &run, results)) failed = 1;
    free (run.blocks); free (run.floors); free (run.segs);
    LEAVE_DEVICE (hip);
    *made_out = made;
    return failed ? -1 : 0;
}

int resampleProcessSchedulePlanarDevice (Resample *cxt, int numBlocks, const artsample_t *d_input, long inputPitch, const int *numInputFrames,
                                         artsample_t *d_output, long outputPitch, const int *numOutputFrames, const double *ratios,
                                         int flushLast, ResampleResult *results)
{
    if (numBlocks <= 0) return 0;
    for (int k = 0; k < numBlocks; ++k) if (numInputFrames [k] < 0) return -1;
    int made;
    return schedule_one (cxt, numBlocks, d_input, inputPitch, numInputFrames, d_output, outputPitch, numOutputFrames, ratios, flushLast, results, &made) ? -1 : made;
}

int resampleProcessScheduleInterleavedDevice (Resample *cxt, int numBlocks, const artsample_t *d_input, const int *numInputFrames,
                                              artsample_t *d_output, const int *numOutputFrames, const double *ratios,
                                              int flushLast, ResampleResult *results)
{
    return resampleProcessSchedulePlanarDevice (cxt, numBlocks, d_input, 0, numInputFrames, d_output, 0, numOutputFrames, ratios, flushLast, results);
}

/* ---- the block schedules of many streams, one launch ------------------------------------------------------------------
 * N drifting streams with K buffered blocks each: a schedule per stream is N launches, a batch per block index K.  The entries below go in
 * ROUNDS.  In a round every live stream that may share a launch plans its next maximal run of gatherable blocks on its context, exactly as
 * its single schedule would (sched_gather, unchanged: the same cuts); the round's runs go out together, one launch per kernel variant
 * (arthip_fir_schedule_batch: every run keeps its own tile, the rolls ride along, one table upload); then every stream whose next block is
 * not gatherable makes it as its single call.  A context that shares no launch is its own single schedule, made first. */
typedef struct {
    SchedRun run;
    size_t in_pos, out_pos;              /* frames in front of the next block, in the stream's input and output */
    int next;                            /* the next block to plan */
    int live;                            /* blocks left to make */
    int cut;                             /* the run was cut at RUN_FRAMES_MAX: its next block is the next round's first */
} SchedStream;

/* what the batch entries refuse before anything is touched (n > 0): a NULL context, one listed twice, a negative frame count */
static int schedule_refused (Resample *const *cxts, int n, const int *numBlocks, const int *const *numInputFrames)
{
    if (artamd_batch_distinct ((const void *const *) cxts, n, stamp_of, "resample schedule", "context")) return -1;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < numBlocks [i]; ++k) if (numInputFrames [i] [k] < 0) return -1;
    return 0;
}

static int schedule_batch (Resample *const *cxts, int n, const int *numBlocks, const artsample_t *const *d_inputs, const long *in_pitches,
                           const int *const *numInputFrames, artsample_t *const *d_outputs, const long *out_pitches,
                           const int *const *numOutputFrames, const double *const *ratios, const int *flushLast,
                           ResampleResult *const *results, int *blocksMade)
{
    if (n <= 0) return 0;
    if (schedule_refused (cxts, n, numBlocks, numInputFrames)) return -1;

    struct artamd_resampler *lead = cxts [0]->hip;
    SchedStream *st = calloc ((size_t) n, sizeof (SchedStream));
    ArtSchedItem *items = malloc (sizeof (ArtSchedItem) * (size_t) n);
    int *item_of = malloc (sizeof (int) * (size_t) n);
    int launches = 0, failed = 0, live = 0;

    for (int i = 0; i < n; ++i) {
        blocksMade [i] = 0;
        if (numBlocks [i] > 0) zero_results (results [i], NULL, numBlocks [i]);
    }
    if (!st || !items || !item_of) { free (st); free (items); free (item_of); artamd_note_failure ("resampler: out of memory (schedule batch)"); return -1; }

    ENTER_DEVICE (lead);
    for (int i = 0; i < n && !failed; ++i) {
        Resample *cxt = cxts [i];
        if (numBlocks [i] <= 0) continue;
        if (shares_lead (cxt, lead) && !(cxt->flags & RESAMPLE_STRICT_ORDER)) { st [i].live = 1; ++live; continue; }
        /* (sharded, another stream or device, timing on; strict order, which gathers nothing: the context's own schedule) */
        failed = schedule_one (cxt, numBlocks [i], d_inputs [i], in_pitches ? in_pitches [i] : 0, numInputFrames [i], d_outputs [i],
                               out_pitches ? out_pitches [i] : 0, numOutputFrames [i], ratios [i], flushLast ? flushLast [i] : 0, results [i], &blocksMade [i]);
        ++launches;
    }

    while (live && !failed) {
        int nitems = 0, nb = 0, ns = 0;
        /* every live stream's next run */
        for (int i = 0; i < n; ++i) {
            SchedStream *s = &st [i];
            if (!s->live) continue;
            Resample *cxt = cxts [i];
            const int C = cxt->numChannels;
            const long in_pitch = in_pitches ? in_pitches [i] : 0, out_pitch = out_pitches ? out_pitches [i] : 0;
            s->cut = 0;
            while (s->next < numBlocks [i]) {
                const int k = s->next, nIn = numInputFrames [i] [k];
                if (flushLast && flushLast [i] && k == numBlocks [i] - 1) break;
                if (s->run.gathered && s->run.frames > RUN_FRAMES_MAX - nIn) { s->cut = 1; break; }
                if (!sched_gather (cxt, &s->run, sched_at (d_inputs [i], in_pitch, s->in_pos, C), in_pitch, nIn,
                                   (art_s *) sched_at (d_outputs [i], out_pitch, s->out_pos, C), out_pitch, numOutputFrames [i] [k], ratios [i] [k],
                                   &results [i] [k], k)) break;
                ++s->next;
                if ((int) results [i] [k].input_used != nIn) { s->next = numBlocks [i]; break; }       /* a cap too small: no later block is made */
                s->in_pos += (size_t) nIn; s->out_pos += results [i] [k].output_generated;
            }
            if (s->run.nblocks) {
                ArtSchedItem *it = &items [nitems];
                sched_run_args (cxt, &s->run, &it->run);
                it->blocks = s->run.blocks; it->nblocks = s->run.nblocks; it->segs = s->run.segs; it->nsegs = s->run.nsegs; it->launched = 0;
                nb += it->nblocks; ns += it->nsegs;
                item_of [i] = nitems++;
            }
        }
        /* the round's runs, one launch per kernel variant */
        int rc = 0;
        if (nitems) {
            lead->d_sched_batch = arthip_grow (lead->d_sched_batch, &lead->sched_batch_cap, arthip_fir_schedule_batch_bytes (nitems, nb, ns));
            rc = lead->d_sched_batch ? arthip_fir_schedule_batch (items, nitems, lead->d_sched_batch, lead->stream) : -1;
            if (rc < 0) {
                fprintf (stderr, "artamd: resample schedule batch launch failed: %s\n", arthip_last_error ());
                artamd_note_failure ("resampler: schedule batch launch failed");
                failed = 1;
            }
            else launches += rc;
        }
        for (int i = 0; i < n; ++i) {
            SchedStream *s = &st [i];
            if (!s->live || !s->run.gathered) continue;
            const int first = s->run.first, gathered = s->run.gathered, launched = s->run.nblocks && items [item_of [i]].launched;
            if (failed && !launched) {
                /* (the stream stands where it stood before its run; no later block of it is made) */
                sched_run_undo (cxts [i], &s->run, results [i]);
                if (first + gathered < numBlocks [i]) zero_results (results [i] + first + gathered, NULL, numBlocks [i] - first - gathered);
                continue;
            }
            if (!s->run.nblocks && s->run.frames > 0) ++launches;                    /* (no output: the history roll alone) */
            sched_run_done (cxts [i], &s->run, launched, launched);
            blocksMade [i] = first + gathered;
        }
        if (failed) break;
        /* the blocks that are single calls, behind their streams' runs */
        for (int i = 0; i < n && !failed; ++i) {
            SchedStream *s = &st [i];
            if (!s->live) continue;
            if (s->next < numBlocks [i] && !s->cut) {
                Resample *cxt = cxts [i];
                const int C = cxt->numChannels, k = s->next, nIn = numInputFrames [i] [k];
                const long in_pitch = in_pitches ? in_pitches [i] : 0, out_pitch = out_pitches ? out_pitches [i] : 0;
                const int errors = artamdErrorCount ();
                results [i] [k] = sched_single (cxt, sched_at (d_inputs [i], in_pitch, s->in_pos, C), in_pitch, nIn,
                                                (art_s *) sched_at (d_outputs [i], out_pitch, s->out_pos, C), out_pitch, numOutputFrames [i] [k], ratios [i] [k],
                                                flushLast && flushLast [i] && k == numBlocks [i] - 1);
                ++launches;
                if (artamdErrorCount () != errors) { zero_results (&results [i] [k], NULL, 1); failed = 1; break; }
                blocksMade [i] = ++s->next;
                if ((int) results [i] [k].input_used != nIn) s->next = numBlocks [i];
                s->in_pos += (size_t) nIn; s->out_pos += results [i] [k].output_generated;
            }
            if (s->next >= numBlocks [i]) { s->live = 0; --live; }
        }
    }
    LEAVE_DEVICE (lead);
    for (int i = 0; i < n; ++i) { free (st [i].run.blocks); free (st [i].run.floors); free (st [i].run.segs); }
    free (st); free (items); free (item_of);
    return failed ? -1 : launches;
}

int resampleProcessScheduleBatchInterleavedDevice (Resample *const *cxts, int n, const int *numBlocks,
        const artsample_t *const *d_inputs, const int *const *numInputFrames,
        artsample_t *const *d_outputs, const int *const *numOutputFrames, const double *const *ratios,
        const int *flushLast, ResampleResult *const *results, int *blocksMade)
{
    return schedule_batch (cxts, n, numBlocks, d_inputs, NULL, numInputFrames, d_outputs, NULL, numOutputFrames, ratios, flushLast, results, blocksMade);
}

int resampleProcessScheduleBatchPlanarDevice (Resample *const *cxts, int n, const int *numBlocks,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *const *numInputFrames,
        artsample_t *const *d_outputs, const long *outputPitches, const int *const *numOutputFrames,
        const double *const *ratios, const int *flushLast, ResampleResult *const *results, int *blocksMade)
{
    return schedule_batch (cxts, n, numBlocks, d_inputs, inputPitches, numInputFrames, d_outputs, outputPitches, numOutputFrames, ratios, flushLast, results, blocksMade);
}

/* ... whole clips from a fresh start: the contexts put back as resampleProcessAndFlushClipsPlanarDevice puts them back (batch_from_start), after
 * the schedule's own refusals and in front of its launches */
int resampleProcessScheduleClipsPlanarDevice (Resample *const *cxts, int n, const int *numBlocks,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *const *numInputFrames,
        artsample_t *const *d_outputs, const long *outputPitches, const int *const *numOutputFrames,
        const double *const *ratios, const int *flushLast, int fromStart, ResampleResult *const *results, int *blocksMade)
{
    int zeroing = 0;
    if (fromStart && n > 0) {
        if (schedule_refused (cxts, n, numBlocks, numInputFrames)) return -1;       /* (schedule_batch asks again: the same list) */
        struct artamd_resampler *lead = cxts [0]->hip;
        ENTER_DEVICE (lead);
        const int failed = batch_from_start (cxts, n);
        LEAVE_DEVICE (lead);
        if (failed) {
            artamd_note_failure ("resampler: the schedule clips entry could not put its contexts back (nothing enqueued)");
            return -1;
        }
        /* (the zeroing launch: made if a context shares it — batch_from_start's own condition) */
        for (int i = 0; i < n && !zeroing; ++i) {
            const struct artamd_resampler *hip = cxts [i]->hip;
            zeroing = !hip->nshards && hip->stream == lead->stream && hip->device == lead->device;
        }
    }
    const int rc = schedule_batch (cxts, n, numBlocks, d_inputs, inputPitches, numInputFrames, d_outputs, outputPitches, numOutputFrames, ratios, flushLast, results, blocksMade);
    return rc < 0 ? -1 : rc + zeroing;
}

/* what a call would consume / produce, without touching the context */
static ResampleResult peek_call (Resample *cxt, int nIn, int cap, double ratio)
{
    ResampleResult peek;
    ArtamdPosition pos = position_of (cxt);
    int dummy_floor;

    artamdPlanCall (&pos, nIn, cap, ratio, &peek, NULL, 0, &dummy_floor);
    return peek;
}

/* a sharded context mirrors the position of its shards (they all hold the same one) */
static ResampleResult shards_agree (Resample *cxt, const ResampleResult *per_shard)
{
    struct artamd_resampler *hip = cxt->hip;
    const Resample *first = hip->shards [0];
    ResampleResult res = per_shard [0];

    for (int k = 1; k < hip->nshards; ++k)
        if (per_shard [k].input_used != res.input_used || per_shard [k].output_generated != res.output_generated ||
            hip->shards [k]->inputIndex != first->inputIndex || hip->shards [k]->outputOffset != first->outputOffset) {
            fprintf (stderr, "artamd: sharded context: shard %d disagrees with shard 0 (a launch failed?)\n", k);
            zero_results (&res, NULL, 1);
        }
    cxt->outputOffset = first->outputOffset; cxt->inputIndex = first->inputIndex;
    cxt->flags = first->flags | RESAMPLE_MULTITHREADED;
    return res;
}

/* Device-pointer call on a sharded context: the caller's buffers live on the context's own device; every shard pulls its
 * channel slice (strided rows, peer-to-peer over xGMI when the shard sits on another GPU), runs, and pushes its slice of
 * the output back.  Ordered after the context's stream, and the context's stream continues only when all shards are done.
 * Planar buffers need no copies at all: a shard's channels are a contiguous run of planes.
 * A shard's part is six or seven enqueues (wait, slice in, staging / prepare, FIR, slice out, record): ~20 us of host time.  One
 * after the other from the calling thread that is 160 us per call on eight devices — more than a 4-channel shard's 1M-frame call
 * takes on its GPU — so every shard has a WORKER THREAD (round 3's verdict): the caller posts the call's arguments, the workers
 * enqueue their shards side by side (each on its own device and stream; the HIP runtime is entered from several threads at once,
 * which it allows), the caller waits for the enqueues — not the GPUs — and lets the context's stream wait for the shards' events.
 * (Where the shards sit on one device the calling thread does it all, as in rounds 2-3: shard_pool_create.) */
struct shard_job {
    const art_s *d_in; long in_pitch; int nIn; art_s *d_out; long out_pitch; int cap; double ratio;
    ResampleResult peek;
};

static ResampleResult shard_part (Resample *cxt, int k, const struct shard_job *j, int *failed)
{
    struct artamd_resampler *hip = cxt->hip;
    Resample *sh = hip->shards [k];
    struct artamd_resampler *sp = sh->hip;
    const int C = cxt->numChannels, first = hip->shard_first [k], width = sh->numChannels;
    ResampleResult res = { 0, 0 };

    arthip_set_device (sp->device);
    arthip_stream_wait_event (sp->stream, hip->ev_parent);
    if (j->in_pitch && j->out_pitch)
        res = enqueue_call_layouts (sh, j->d_in ? j->d_in + (size_t) first * j->in_pitch : NULL, j->in_pitch, j->nIn,
                                    j->d_out + (size_t) first * j->out_pitch, j->out_pitch, j->cap, j->ratio);
    else if (j->in_pitch || j->out_pitch) {
        /* one side planar, the other interleaved (a pitch of 0): the planar side is the shard's own run of planes; the interleaved side
         * is a strided slice of the caller's stream-wide frames and goes through the shard's slice staging, as in the branch below */
        const int wpw = (int)(sizeof (art_s) / 4);
        if (j->out_pitch) {                                     /* interleaved in, planar out */
            sp->d_in = arthip_grow (sp->d_in, &sp->in_cap, sizeof (art_s) * (size_t) j->peek.input_used * width);
            if (j->peek.input_used && !sp->d_in) { *failed = 1; arthip_event_record (hip->ev_shard [k], sp->stream); return res; }
            if (j->peek.input_used && j->d_in)
                arthip_slice_copy (sp->d_in, (size_t) width * wpw, j->d_in + first, (size_t) C * wpw, width * wpw, j->peek.input_used, sp->stream);
            res = enqueue_call_layouts (sh, j->d_in ? sp->d_in : NULL, 0, j->nIn, j->d_out + (size_t) first * j->out_pitch, j->out_pitch, j->cap, j->ratio);
        }
        else {                                                  /* planar in, interleaved out */
            sp->d_out = arthip_grow (sp->d_out, &sp->out_cap, sizeof (art_s) * ((size_t) j->peek.output_generated + 16) * width);
            if (j->peek.output_generated && !sp->d_out) { *failed = 1; arthip_event_record (hip->ev_shard [k], sp->stream); return res; }
            res = enqueue_call_layouts (sh, j->d_in ? j->d_in + (size_t) first * j->in_pitch : NULL, j->in_pitch, j->nIn, sp->d_out, 0, j->cap, j->ratio);
            if (res.output_generated)
                arthip_slice_copy (j->d_out + first, (size_t) C * wpw, sp->d_out, (size_t) width * wpw, width * wpw, res.output_generated, sp->stream);
        }
    }
    else {
        sp->d_in = arthip_grow (sp->d_in, &sp->in_cap, sizeof (art_s) * (size_t) j->peek.input_used * width);
        sp->d_out = arthip_grow (sp->d_out, &sp->out_cap, sizeof (art_s) * (size_t) j->peek.output_generated * width);
        if ((j->peek.input_used && !sp->d_in) || (j->peek.output_generated && !sp->d_out)) { *failed = 1; arthip_event_record (hip->ev_shard [k], sp->stream); return res; }
        const int wpw = (int)(sizeof (art_s) / 4);              /* 4-byte words per sample */
        if (j->peek.input_used && j->d_in)
            arthip_slice_copy (sp->d_in, (size_t) width * wpw, j->d_in + first, (size_t) C * wpw, width * wpw, j->peek.input_used, sp->stream);
        res = enqueue_call (sh, sp->d_in, 0, j->nIn, sp->d_out, 0, j->cap, j->ratio);
        arthip_slice_copy (j->d_out + first, (size_t) C * wpw, sp->d_out, (size_t) width * wpw, width * wpw, res.output_generated, sp->stream);
    }
    arthip_event_record (hip->ev_shard [k], sp->stream);
    return res;
}

struct shard_pool {
    Resample *cxt;
    int n, quit;
    unsigned long call;                      /* number of the call the workers are to make (posted under the lock) */
    int pending;                             /* workers that have not finished it yet */
    struct shard_job job;
    ResampleResult res [MAX_DEVICES];
    int failed [MAX_DEVICES];
    char err [MAX_DEVICES] [256];            /* a worker's own error text (arthip_last_error is per thread) for the caller to report */
    pthread_t thread [MAX_DEVICES];
    int started;
    pthread_mutex_t lock;
    pthread_cond_t go, done;
};

struct shard_worker_arg { struct shard_pool *pool; int k; };

static void *shard_worker (void *p)
{
    struct shard_worker_arg *wa = p;
    struct shard_pool *pool = wa->pool;
    const int k = wa->k;
    unsigned long seen = 0;
    free (wa);
    pthread_mutex_lock (&pool->lock);
    for (;;) {
        while (!pool->quit && pool->call == seen) pthread_cond_wait (&pool->go, &pool->lock);
        if (pool->quit) break;
        seen = pool->call;
        pthread_mutex_unlock (&pool->lock);
        pool->failed [k] = 0;
        arthip_set_last_error (NULL);
        pool->res [k] = shard_part (pool->cxt, k, &pool->job, &pool->failed [k]);
        snprintf (pool->err [k], sizeof (pool->err [k]), "%s", arthip_last_error ());
        pthread_mutex_lock (&pool->lock);
        if (--pool->pending == 0) pthread_cond_signal (&pool->done);
    }
    pthread_mutex_unlock (&pool->lock);
    return NULL;
}

static struct shard_pool *shard_pool_create (Resample *cxt, int n)
{
    /* threads where the shards sit on DIFFERENT devices (each device's queue is fed by its own thread); several shards on one device
     * — ARTAMD_SHARDS on a one-GPU box — are enqueued by the caller: eight threads entering the runtime for one device contend for
     * it (measured, tools/bench_sharded_context.py, 16,384-frame calls: 231 us with threads, 205 without).  ARTAMD_SHARD_THREADS=1 /
     * =0 forces either. */
    const char *e = getenv ("ARTAMD_SHARD_THREADS");
    int distinct = 0;
    for (int k = 0; k < n; ++k) {
        int seen = 0;
        for (int i = 0; i < k; ++i) seen |= cxt->hip->shards [i]->hip->device == cxt->hip->shards [k]->hip->device;
        distinct += !seen;
    }
    if (n < 2 || (e && *e == '0') || (distinct < 2 && !(e && *e == '1'))) return NULL;
    struct shard_pool *pool = calloc (1, sizeof (*pool));
    if (!pool) return NULL;
    pool->cxt = cxt; pool->n = n;
    pthread_mutex_init (&pool->lock, NULL); pthread_cond_init (&pool->go, NULL); pthread_cond_init (&pool->done, NULL);
    for (int k = 0; k < n; ++k) {
        struct shard_worker_arg *wa = malloc (sizeof (*wa));
        if (!wa) break;
        wa->pool = pool; wa->k = k;
        if (pthread_create (&pool->thread [k], NULL, shard_worker, wa)) { free (wa); break; }
        pool->started = k + 1;
    }
    if (pool->started != n) { shard_pool_destroy (pool); return NULL; }
    return pool;
}

static void shard_pool_destroy (struct shard_pool *pool)
{
    if (!pool) return;
    pthread_mutex_lock (&pool->lock);
    pool->quit = 1;
    pthread_cond_broadcast (&pool->go);
    pthread_mutex_unlock (&pool->lock);
    for (int k = 0; k < pool->started; ++k) pthread_join (pool->thread [k], NULL);
    pthread_mutex_destroy (&pool->lock); pthread_cond_destroy (&pool->go); pthread_cond_destroy (&pool->done);
    free (pool);
}

static ResampleResult sharded_device_call (Resample *cxt, const art_s *d_in, long in_pitch, int nIn, art_s *d_out, long out_pitch,
                                           int cap, double ratio)
{
    struct artamd_resampler *hip = cxt->hip;
    const int prev = arthip_current_device ();
    ResampleResult per_shard [MAX_DEVICES], res = { 0, 0 };
    int failed = 0;
    struct shard_job job = { d_in, in_pitch, nIn, d_out, out_pitch, cap, ratio, peek_call (cxt, nIn, cap, ratio) };

    arthip_set_device (hip->device);
    arthip_event_record (hip->ev_parent, hip->stream);

    struct shard_pool *pool = hip->pool;
    if (pool) {
        pthread_mutex_lock (&pool->lock);
        pool->job = job; pool->pending = pool->n; ++pool->call;
        pthread_cond_broadcast (&pool->go);
        while (pool->pending) pthread_cond_wait (&pool->done, &pool->lock);
        pthread_mutex_unlock (&pool->lock);
        for (int k = 0; k < hip->nshards; ++k) {
            per_shard [k] = pool->res [k]; failed |= pool->failed [k];
            /* (a worker that failed, or whose launch made nothing where shard 0's made something: its thread's error text becomes this thread's) */
            if (pool->failed [k] || per_shard [k].output_generated != pool->res [0].output_generated) arthip_set_last_error (pool->err [k]);
        }
    }
    else
        for (int k = 0; k < hip->nshards; ++k) { int f = 0; per_shard [k] = shard_part (cxt, k, &job, &f); failed |= f; }

    arthip_set_device (hip->device);
    for (int k = 0; k < hip->nshards; ++k)
        arthip_stream_wait_event (hip->stream, hip->ev_shard [k]);
    if (prev >= 0) arthip_set_device (prev);

    res = shards_agree (cxt, per_shard);
    if (failed) { artamd_note_failure ("resampler: sharded context: device allocation failed"); zero_results (&res, NULL, 1); }
    return res;
}

/* Does a device-pointer call of these layouts go through the context's interleaved staging buffers (enqueue_call_layouts, and the planar batch
 * entries, which decide for every context as its single call would)? */
static int staged_layouts (const Resample *cxt, const art_s *d_in, long in_pitch, int nIn, const art_s *d_out, long out_pitch, int cap)
{
    const struct artamd_resampler *hip = cxt->hip;
    return (in_pitch || out_pitch) && nIn > 0 && cap > 0 && d_in && d_out &&
           ((double) nIn * (hip->stream_channels > cxt->numChannels ? hip->stream_channels : cxt->numChannels) * cxt->numTaps >= 2.0e8 ||       /* (a shard: its whole stream's size) */
            hip->kernel_pref == ART_KERNEL_INVARIANT);           /* (the cut-invariant policy: every call, whatever its size, on the same kernel) */
}

/* enqueue_call for device buffers of either layout (the context's device is current) */
static ResampleResult enqueue_call_layouts (Resample *cxt, const art_s *d_in, long in_pitch, int nIn, art_s *d_out, long out_pitch, int cap, double ratio)
{
    struct artamd_resampler *hip = cxt->hip;
    /* Planar device buffers.  The matrix-core path reads and writes interleaved frames only, and a big planar call on the general
     * kernel is 4-7 x slower than the same call interleaved (8 ch x 988 taps, 1M frames: 960 against 140 us).  Such a call goes
     * through the context's interleaved staging buffers — two transposing copies on the device, ~4 % of the call — and so does a
     * call with only one planar side.  (Small calls stay as they are: the general kernel takes planes as they come.) */
    if (staged_layouts (cxt, d_in, in_pitch, nIn, d_out, out_pitch, cap)) {
        const int C = cxt->numChannels;
        const art_s *in_i = d_in; art_s *out_i = d_out;
        int ok = 1;
        if (in_pitch) {
            hip->d_in = arthip_grow (hip->d_in, &hip->in_cap, sizeof (art_s) * (size_t) nIn * C);
            ok = hip->d_in && !arthip_interleave (hip->d_in, d_in, in_pitch, nIn, C, hip->stream);
            in_i = hip->d_in;
        }
        if (ok && out_pitch) {
            /* (room for the frames the call will make, not for the caller's whole capacity) */
            const ResampleResult pk = peek_call (cxt, nIn, cap, ratio);
            hip->d_out = arthip_grow (hip->d_out, &hip->out_cap, sizeof (art_s) * ((size_t) pk.output_generated + 16) * C);
            ok = hip->d_out != NULL;
            out_i = hip->d_out;
        }
        if (ok) {
            const ResampleResult res = enqueue_call (cxt, in_i, 0, nIn, out_i, 0, cap, ratio);
            if (out_pitch && res.output_generated) arthip_deinterleave (d_out, out_pitch, out_i, (int) res.output_generated, C, hip->stream);
            return res;
        }
    }
    return enqueue_call (cxt, d_in, in_pitch, nIn, d_out, out_pitch, cap, ratio);
}

static ResampleResult device_call (Resample *cxt, const art_s *d_in, long in_pitch, int nIn, art_s *d_out, long out_pitch, int cap, double ratio)
{
    struct artamd_resampler *hip = cxt->hip;
    if (hip->nshards) return sharded_device_call (cxt, d_in, in_pitch, nIn, d_out, out_pitch, cap, ratio);
    ENTER_DEVICE (hip);
    const ResampleResult res = enqueue_call_layouts (cxt, d_in, in_pitch, nIn, d_out, out_pitch, cap, ratio);
    LEAVE_DEVICE (hip);
    return res;
}

ResampleResult resampleProcessInterleavedDevice (Resample *cxt, const artsample_t *d_input, int numInputFrames,
                                                 artsample_t *d_output, int numOutputFrames, double ratio)
{
    return device_call (cxt, d_input, 0, numInputFrames, d_output, 0, numOutputFrames, ratio);
}

ResampleResult resampleProcessPlanarDevice (Resample *cxt, const artsample_t *d_input, long inputPitch, int numInputFrames,
                                            artsample_t *d_output, long outputPitch, int numOutputFrames, double ratio)
{
    return device_call (cxt, d_input, inputPitch, numInputFrames, d_output, outputPitch, numOutputFrames, ratio);
}

ResampleResult resampleProcessAndFlushInterleavedDevice (Resample *cxt, const artsample_t *d_input, int numInputFrames,
                                                         artsample_t *d_output, int numOutputFrames, double ratio)
{
    ResampleResult res = resampleProcessInterleavedDevice (cxt, d_input, numInputFrames, d_output, numOutputFrames, ratio);

    if ((numInputFrames -= res.input_used) != 0 || (numOutputFrames -= res.output_generated) == 0)
        return res;

    ResampleResult tail = resampleProcessInterleavedDevice (cxt, NULL, -1, d_output + (size_t) res.output_generated * cxt->numChannels,
                                                            numOutputFrames, ratio);
    res.output_generated += tail.output_generated;
    return res;
}

/* (the flush writes behind the process call's frames: in every plane of a planar output) */
ResampleResult resampleProcessAndFlushPlanarDevice (Resample *cxt, const artsample_t *d_input, long inputPitch, int numInputFrames,
                                                    artsample_t *d_output, long outputPitch, int numOutputFrames, double ratio)
{
    ResampleResult res = resampleProcessPlanarDevice (cxt, d_input, inputPitch, numInputFrames, d_output, outputPitch, numOutputFrames, ratio);

    if ((numInputFrames -= res.input_used) != 0 || (numOutputFrames -= res.output_generated) == 0)
        return res;

    ResampleResult tail = resampleProcessPlanarDevice (cxt, NULL, inputPitch, -1, d_output + (size_t) res.output_generated * (outputPitch ? 1 : cxt->numChannels),
                                                       outputPitch, numOutputFrames, ratio);
    res.output_generated += tail.output_generated;
    return res;
}

/* ------------------------------------------------------------------------------------------
 * Host-pointer calls (what ART and artest use).  host_begin stages the call's input in HBM, enqueues the call and starts
 * the copy back; host_end waits and delivers.  A sharded context begins on all its shards before it ends any, so the
 * devices work side by side.  The caller's frames are `in_stride` / `out_stride` samples apart (a shard sees its channel
 * slice of a wider stream: the de-interleaving happens on the way into its HBM).
 *   up to STAGE_LIMIT bytes: packed by the CPU into page-locked staging, ONE dense DMA each way;
 *   beyond: straight from / to the caller's memory (strided rows: a 2-D copy), the runtime pipelines the pages.
 * ---------------------------------------------------------------------------------------- */
typedef struct { ResampleResult res; int staged_out, failed; } HostPending;

/* ARTAMD_HOST_TRACE=1: where a host-pointer call spends its time (host clock, accumulated, printed by resampleFree) */
static double trace_acc [8]; static long trace_calls;
static inline double trace_now (void) { struct timespec ts; clock_gettime (CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }
#define TRACE_MARK(slot) do { if (trace_on > 0) { const double now_ = trace_now (); trace_acc [slot] += now_ - trace_t_; trace_t_ = now_; } } while (0)
static void trace_report (void)
{
    if (trace_on > 0 && trace_calls) {
        fprintf (stderr, "artamd host trace, us per call over %ld calls: plan+grow %.1f | pack %.1f | H2D enqueue %.1f | plan+launch %.1f | D2H enqueue %.1f | "
                 "wait %.1f | unpack %.1f\n", trace_calls, trace_acc [0] / trace_calls, trace_acc [1] / trace_calls, trace_acc [2] / trace_calls,
                 trace_acc [3] / trace_calls, trace_acc [4] / trace_calls, trace_acc [5] / trace_calls, trace_acc [6] / trace_calls);
        memset (trace_acc, 0, sizeof (trace_acc)); trace_calls = 0;
    }
}

static void host_begin (Resample *cxt, const art_s *input, int in_stride, const art_s *const *planes, int nIn,
                        art_s *output, int out_stride, art_s *const *out_planes, int cap, double ratio, HostPending *pend)
{
    struct artamd_resampler *hip = cxt->hip;
    const int C = cxt->numChannels;
    const ResampleResult peek = peek_call (cxt, nIn, cap, ratio);
    const size_t in_samples = (size_t) peek.input_used * C, out_samples = (size_t) peek.output_generated * C;
    const char *limit_env = getenv ("ARTAMD_STAGE_LIMIT");
    const int staged = sizeof (art_s) * (in_samples + out_samples) <= (limit_env && *limit_env ? (size_t) strtoull (limit_env, NULL, 10) : STAGE_LIMIT);

    zero_results (&pend->res, NULL, 1); pend->staged_out = 0; pend->failed = 1;
    if (trace_on < 0) { const char *e = getenv ("ARTAMD_HOST_TRACE"); trace_on = e && *e && *e != '0'; if (trace_on) atexit (trace_report); }
    double trace_t_ = trace_on > 0 ? trace_now () : 0.0;
    trace_calls += trace_on > 0;

    hip->d_in = arthip_grow (hip->d_in, &hip->in_cap, sizeof (art_s) * in_samples);
    hip->d_out = arthip_grow (hip->d_out, &hip->out_cap, sizeof (art_s) * out_samples);
    if (staged) {
        hip->h_in = grow_pinned (hip->h_in, &hip->h_in_cap, sizeof (art_s) * in_samples);
        hip->h_out = grow_pinned (hip->h_out, &hip->h_out_cap, sizeof (art_s) * out_samples);
    }
    else if (planes || out_planes) {
        const size_t big = in_samples > out_samples ? in_samples : out_samples;
        hip->d_tmp = arthip_grow (hip->d_tmp, &hip->tmp_cap, sizeof (art_s) * big);
    }
    if ((in_samples && !hip->d_in) || (out_samples && !hip->d_out) || (staged && ((in_samples && !hip->h_in) || (out_samples && !hip->h_out))) ||
        (!staged && (planes || out_planes) && !hip->d_tmp)) {
        fprintf (stderr, "artamd: staging allocation failed: %s\n", arthip_last_error ());
        return;
    }

    TRACE_MARK (0);
    if (in_samples && staged) {
        art_s *dst = hip->h_in;
        if (planes)
            for (int c = 0; c < C; ++c) {
                const art_s *src = planes [c];
                for (unsigned int f = 0; f < peek.input_used; ++f) dst [(size_t) f * C + c] = src [f];
            }
        else if (in_stride == C)
            memcpy (dst, input, sizeof (art_s) * in_samples);
        else
            for (unsigned int f = 0; f < peek.input_used; ++f) {
                const art_s *row = input + (size_t) f * in_stride;
                for (int c = 0; c < C; ++c) dst [(size_t) f * C + c] = row [c];
            }
        TRACE_MARK (1);
        if (sizeof (art_s) * in_samples <= KERNEL_COPY_LIMIT) arthip_copy_by_kernel (hip->d_in, hip->h_in, sizeof (art_s) * in_samples, hip->stream);
        else arthip_h2d (hip->d_in, hip->h_in, sizeof (art_s) * in_samples, hip->stream);
    }
    else if (in_samples) {
        if (planes) {
            for (int c = 0; c < C; ++c)
                arthip_h2d (hip->d_tmp + (size_t) c * peek.input_used, planes [c], sizeof (art_s) * peek.input_used, hip->stream);
            arthip_interleave (hip->d_in, hip->d_tmp, peek.input_used, (int) peek.input_used, C, hip->stream);
        }
        else if (in_stride == C)
            arthip_h2d (hip->d_in, input, sizeof (art_s) * in_samples, hip->stream);
        else
            arthip_copy2d (hip->d_in, sizeof (art_s) * C, input, sizeof (art_s) * in_stride, sizeof (art_s) * C, peek.input_used, hip->stream);
    }

    TRACE_MARK (2);
    /* small staged calls: the FIR kernels write their output straight into the page-locked buffer (it is mapped into the
     * device's address space; one launch and its dependency gap less than copying it out afterwards) */
    const int direct_out = staged && sizeof (art_s) * out_samples <= DIRECT_OUT_LIMIT && !hip->nshards;
    pend->res = hip->nshards ? sharded_device_call (cxt, hip->d_in, 0, nIn, hip->d_out, 0, cap, ratio)
                             : enqueue_call (cxt, hip->d_in, 0, nIn, direct_out ? hip->h_out : hip->d_out, 0, cap, ratio);
    pend->failed = 0;
    TRACE_MARK (3);

    const unsigned int made = pend->res.output_generated;
    if (!made) return;
    if (staged) {
        if (!direct_out) {
            if (sizeof (art_s) * (size_t) made * C <= KERNEL_COPY_LIMIT) arthip_copy_by_kernel (hip->h_out, hip->d_out, sizeof (art_s) * (size_t) made * C, hip->stream);
            else arthip_d2h (hip->h_out, hip->d_out, sizeof (art_s) * (size_t) made * C, hip->stream);
        }
        pend->staged_out = 1;
    }
    else if (out_planes) {
        arthip_deinterleave (hip->d_tmp, made, hip->d_out, (int) made, C, hip->stream);
        for (int c = 0; c < C; ++c)
            arthip_d2h (out_planes [c], hip->d_tmp + (size_t) c * made, sizeof (art_s) * made, hip->stream);
    }
    else if (out_stride == C)
        arthip_d2h (output, hip->d_out, sizeof (art_s) * (size_t) made * C, hip->stream);
    else
        arthip_copy2d (output, sizeof (art_s) * out_stride, hip->d_out, sizeof (art_s) * C, sizeof (art_s) * C, made, hip->stream);
    TRACE_MARK (4);
}

static void host_end (Resample *cxt, art_s *output, int out_stride, art_s *const *out_planes, const HostPending *pend)
{
    struct artamd_resampler *hip = cxt->hip;
    const int C = cxt->numChannels;
    const unsigned int made = pend->res.output_generated;

    double trace_t_ = trace_on > 0 ? trace_now () : 0.0;
    arthip_sync (hip->stream);
    TRACE_MARK (5);
    if (!pend->staged_out || !made) return;

    const art_s *src = hip->h_out;
    if (out_planes)
        for (int c = 0; c < C; ++c) {
            art_s *dst = out_planes [c];
            for (unsigned int f = 0; f < made; ++f) dst [f] = src [(size_t) f * C + c];
        }
    else if (out_stride == C)
        memcpy (output, src, sizeof (art_s) * (size_t) made * C);
    else
        for (unsigned int f = 0; f < made; ++f) {
            art_s *row = output + (size_t) f * out_stride;
            for (int c = 0; c < C; ++c) row [c] = src [(size_t) f * C + c];
        }
    TRACE_MARK (6);
}

/* A sharded context stages the WHOLE interleaved buffer on its own device exactly as an ordinary context does (one dense
 * transfer each way at full PCIe rate) and hands it to the device-pointer path, whose shards pull and push their channel
 * slices with slice kernels (peer-to-peer over xGMI when they sit on other GPUs).  (Tried first: every shard packing and
 * uploading its own slice — the 2-D copy command moves 16-byte rows one by one (32 ch x 262,144 frames: 16 ms against 1.5 ms
 * for the dense copy), and CPU packing reads the whole interleaved buffer once per shard.) */
static ResampleResult host_call (Resample *cxt, const art_s *input, const art_s *const *planes, int nIn,
                                 art_s *output, art_s *const *out_planes, int cap, double ratio)
{
    struct artamd_resampler *hip = cxt->hip;
    const int C = cxt->numChannels;
    HostPending pend;

    ENTER_DEVICE (hip);
    host_begin (cxt, input, C, planes, nIn, output, C, out_planes, cap, ratio, &pend);
    host_end (cxt, output, C, out_planes, &pend);
    LEAVE_DEVICE (hip);
    return pend.res;
}

ResampleResult resampleProcessInterleaved (Resample *cxt, const artsample_t *input, int numInputFrames, artsample_t *output, int numOutputFrames, double ratio)
{
    return host_call (cxt, input, NULL, numInputFrames, output, NULL, numOutputFrames, ratio);
}

ResampleResult resampleProcess (Resample *cxt, const artsample_t *const *input, int numInputFrames, artsample_t *const *output, int numOutputFrames, double ratio)
{
    return host_call (cxt, NULL, input, numInputFrames, NULL, output, numOutputFrames, ratio);
}

ResampleResult resampleProcessAndFlushInterleaved (Resample *cxt, const artsample_t *input, int numInputFrames, artsample_t *output, int numOutputFrames, double ratio)
{
    ResampleResult res = resampleProcessInterleaved (cxt, input, numInputFrames, output, numOutputFrames, ratio);

    /* unconsumed input or no room left: the caller made a mistake, report what happened */
    if ((numInputFrames -= res.input_used) != 0 || (numOutputFrames -= res.output_generated) == 0)
        return res;

    ResampleResult tail = resampleProcessInterleaved (cxt, NULL, -1, output + (size_t) res.output_generated * cxt->numChannels, numOutputFrames, ratio);
    res.output_generated += tail.output_generated;
    return res;
}

ResampleResult resampleProcessAndFlush (Resample *cxt, const artsample_t *const *input, int numInputFrames, artsample_t *const *output, int numOutputFrames, double ratio)
{
    ResampleResult res = resampleProcess (cxt, input, numInputFrames, output, numOutputFrames, ratio);

    if ((numInputFrames -= res.input_used) != 0 || (numOutputFrames -= res.output_generated) == 0)
        return res;

    art_s **shifted = malloc (sizeof (art_s *) * (size_t) cxt->numChannels);
    for (int c = 0; c < cxt->numChannels; ++c)
        shifted [c] = output [c] + res.output_generated;

    ResampleResult tail = resampleProcess (cxt, NULL, -1, shifted, numOutputFrames, ratio);
    res.output_generated += tail.output_generated;
    free (shifted);
    return res;
}
