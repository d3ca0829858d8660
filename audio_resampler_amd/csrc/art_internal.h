/* art_internal.h — private C ABI between the C host layer (resampler_host.c, pcm_host.c) and the
 * HIP translation units (device_rt.hip, sinc_fir.hip, pcm_kernels.hip).  Plain C types only. */
#ifndef ART_INTERNAL_H
#define ART_INTERNAL_H

#include <stddef.h>
#include <stdint.h>
#include "art_hip.h"

#if defined(PATH_WIDTH) && (PATH_WIDTH==64)
#define ART_WIDE 1          /* double-precision sample path: general + strict kernels only */
#else
#define ART_WIDE 0
#endif
typedef artsample_t art_s;   /* the sample type of this build */

#ifdef __cplusplus
extern "C" {
#endif

/* header of a context's digit-plane buffer (fixed-point matrix kernel, fir_matrix_i8.hip), zeroed when the buffer is allocated:
 * [0] stand-down flag word.  The rows' mask words follow the header. */
#define ART_I8_FLAG_BYTES 256    /* the flag word of the fixed-point kernel's buffer (and what shares its cache line) */
#define ART_I8_HEAD_BYTES 32768  /* the buffer's header, zero when allocated: the flag, then the slab kernel's arrival counters (8 XCDs x 64 tiles x 8 waves) */

#define ART_SPLIT_HEAD_BYTES 65536   /* arrival counters of the K-split kernel: 4 per tile, up to 4096 tiles */
#define ART_MAX_SEGS 192         /* ring-epoch segments per kernel launch (passed by value: 16 B each, kernel arguments stay below 4 KB) */

/* numeric modes of the FIR */
enum { ART_MODE_FAST = 0,        /* f32 FMA accumulation, any order (default) */
       ART_MODE_PRECISE = 1,     /* f64 accumulation (EXTEND_CONVOLUTION_MATH) */
       ART_MODE_STRICT = 2 };    /* reference C source order, un-fused (RESAMPLE_STRICT_ORDER) */

enum { ART_KERNEL_AUTO = 0, ART_KERNEL_GENERAL = 1, ART_KERNEL_MFMA = 2,
       /* the cut-invariant stream policy (art_hip.h, resampleHipSetCutInvariant): ONE arithmetic for every output of a rational-ratio stream however its
        * input is cut into calls — every launch, shorter than a period or not, on the f32 streaming kernel, un-split, anchored on the stream's canonical
        * period; a launch that cannot run anchored is the general kernel's (whose outputs never depend on the cut either) and is counted */
       ART_KERNEL_INVARIANT = 9 };
/* (preferences 6 and 9 both pin the f32 streaming kernel: no fixed point, no K split) */
#define ART_PREF_PINS_F32(k) ((k) == 6 || (k) == ART_KERNEL_INVARIANT)
#define ART_FIR_ROLLED 0x100             /* arthip_fir: the history roll rode along with this launch */

typedef struct {
    int count;
    int lin_floor;                       /* linear indices below this read as silence */
    unsigned int first [ART_MAX_SEGS];   /* first output (call-relative) of each segment, ascending */
    int lin_base [ART_MAX_SEGS];         /* ring index -> linear index (history ++ input) */
    double base [ART_MAX_SEGS];          /* outputOffset of the ring epoch */
} ArtSegTable;

typedef struct {
    const art_s *bank;                   /* device, (F+1) x T */
    const art_s *hist;                   /* device, H frames x C, interleaved */
    const art_s *in;                     /* device, new input frames */
    long in_pitch;                       /* 0: interleaved [frame][C]; else planar, channel c at in + c*in_pitch */
    art_s *out;
    long out_pitch;
    art_s *roll_dst;                     /* when set: the FIR launch also rolls the history (extra workgroups) */
    int roll_appended;                   /*   (frames appended by this call) into roll_dst; arthip_fir then returns k | ART_FIR_ROLLED */                      /* 0: interleaved; else planar */
    int in_frames;                       /* frames valid at `in` (reads beyond return 0) */
    int C, T, F, H;
    int stream_C;                        /* channels of the whole stream when this context is a shard of a multi-device context (0: = C): the
                                          * kernel choice is made for the stream, so that a shard and an ordinary context of the same stream
                                          * run the same kernels and produce the same bits */
    int interpolate, lowpass;            /* SUBSAMPLE_INTERPOLATE / INCLUDE_LOWPASS in effect */
    int mode;                            /* ART_MODE_* */
    double ratio;
    unsigned int n_begin, n_end;         /* call-relative output frames to produce */
    long long lin_origin;                /* stream frame (input frames appended since init / reset, less H) that linear frame 0 of this call is: two calls' linear
                                          * indices differ by the difference of theirs — the rows kept across calls place a launch in the stream's tiling with it */
    int n_skip;                          /* matrix kernels on cached rows (below): the launch's tiles start at the cached period's first slot, n_skip
                                          * slots before the launch's first output — those slots of the first period are computed and not stored */
    int segs_truncated;                  /* the launch reaches beyond the segments of its table (a call of more than ART_MAX_SEGS ring epochs
                                          * handed over whole, ArtFirNeeds.one_launch): only a kernel that follows the lattice from the
                                          * launch's first period may run it — arthip_fir returns -2, nothing enqueued, otherwise */
    /* periodic-phase structure for the MFMA kernel (0 = none): out frame n+period_out sits exactly
     * period_in input frames after out frame n */
    int period_out, period_in;
    /* counters of outputs the matrix kernels evaluated off their slot's canonical pattern (device memory; fix_list is only
     * tested for non-NULL: the path needs the counters) */
    unsigned int *fix_list, *fix_count;
    unsigned int fix_cap;
    /* device scratch for the MFMA path: per-launch effective rows + canonical slot positions */
    void *scratch; size_t scratch_bytes;
    /* device memory for the fixed-point matrix kernel's digit planes of one launch (ArtFirNeeds.planes_bytes; NULL: f32 kernels) */
    void *planes; size_t planes_bytes;
    /* the fixed-point kernel's filter rows ACROSS calls (digit planes, masks, the f32 tables of its stand-by): device memory of
     * ArtFirNeeds.rows_bytes bytes and a zeroed host block of arthip_fir_rows_cache_bytes () bytes that describes what it holds, both owned
     * by the context (NULL: the rows are rebuilt by every launch, as before round 5).  rows_masks_out (host, optional): where the used
     * set's row masks live on the device (resampleHipLastFixedPoint reads them) */
    void *rows; size_t rows_bytes; void *rows_cache; void **rows_masks_out;
    /* device memory for the K-split streaming kernel of launches with few tiles (ArtFirNeeds.split_bytes; NULL: unsplit): the first
     * ART_SPLIT_HEAD_BYTES are arrival counters, zero whenever no launch is in flight (zeroed by the owner when allocated) */
    void *split; size_t split_bytes;
    /* device memory for launches of a channel count the matrix kernels are not compiled for (anything but 1, 2, 4, 8, 16, 32): the
     * launch runs in groups of up to 32 channels, each copied into a buffer of the next compiled width (ArtFirNeeds.pad_bytes; NULL: the
     * generic matrix kernel runs such a stream, several times slower) */
    void *pad; size_t pad_bytes;
    /* host, optional, 4 ints filled when the fixed-point kernel is enqueued: the launch's flag value (the first word of
     * `planes` equals it afterwards iff the kernel stood down), mask words behind the header (at planes + ART_I8_HEAD_BYTES),
     * chunks per tile, the kernel's form (1 register-staged, 2 LDS-DMA, 3 slabs) */
    int *fixed_out;
    /* optional HIP events recorded immediately before/after the dominant kernel's launch (host side only) */
    void *ev_start, *ev_stop;
} ArtFirArgs;

/* ---- device_rt.hip ---- */
int   arthip_device_count (void);
int   arthip_current_device (void);
int   arthip_set_device (int device);
void *arthip_stream_create (void);                         /* non-blocking stream on the current device */
void  arthip_stream_destroy (void *stream);
int   arthip_copy2d (void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, void *stream);   /* any direction */
int   arthip_copy (void *dst, const void *src, size_t bytes, void *stream);                                                /* any direction */
int   arthip_copy_by_kernel (void *dst, const void *src, size_t bytes, void *stream);   /* page-locked host <-> device, small sizes */
int   arthip_copy2_by_kernel (void *dst, const void *src, size_t bytes, void *dst2, const void *src2, size_t bytes2, void *stream);
int   arthip_slice_copy (void *dst, size_t dpitch_words, const void *src, size_t spitch_words, int width_words, size_t rows, void *stream);   /* strided rows of 4-byte words, by a kernel (device / peer memory) */
void *arthip_host_alloc (size_t bytes);                    /* page-locked host memory */
void  arthip_host_free (void *p);
void *arthip_order_event_create (void);                    /* event without timing, for cross-stream ordering */
int   arthip_stream_wait_event (void *stream, void *event);
int   arthip_event_sync (void *event);
int   arthip_enable_peer (int device, int peer);            /* 1: `device` can address `peer`'s memory (or is it); 0: no route */
int   arthip_slice_copy_bytes (void *dst, size_t dpitch, const void *src, size_t spitch, int width, size_t rows, void *stream);   /* strided rows of bytes, by a kernel */
/* copies a host table (bytes) into d_table through the shared pinned staging of the batch launches, on `stream`; 0 or -1 */
int   arthip_table_upload (const void *table, size_t bytes, void *d_table, void *stream);
/* a device buffer of `need` bytes at least: `dev` itself while *cap suffices, else a new, larger one (its content lost) and *cap
 * updated; NULL (and *cap 0) when out of memory */
void *arthip_grow (void *dev, size_t *cap, size_t need);

/* make an object's device (its field `device`) current for the duration of a call; restored afterwards */
#define ENTER_DEVICE(obj) const int prev_device_ = arthip_current_device (); \
                          if (prev_device_ != (obj)->device) arthip_set_device ((obj)->device)
#define LEAVE_DEVICE(obj) do { if (prev_device_ != (obj)->device && prev_device_ >= 0) arthip_set_device (prev_device_); } while (0)

/* ---- resampler_host.c: the device list of multi-device contexts (artamdSetDevices / ARTAMD_DEVICES / ARTAMD_SHARDS) ----
 * how many shards a MULTITHREADED context of `channels` channels gets (0 or 1: an ordinary context) and on which device shard s
 * lives; devices that cannot address `home`'s memory are replaced by `home` */
#define ART_MAX_DEVICES 64
int   artamd_shard_plan (int channels, int home, int *devices_out);
/* the batch calls' check of their list: no item NULL, none named twice (each item's stamp, *stamp_of (item), is set to this call's
 * number: one pass).  0, or -1 with "artamd: <what> batch: a NULL <noun>" or "... a <noun> appears twice" printed */
int   artamd_batch_distinct (const void *const *items, int n, unsigned long *(*stamp_of) (const void *item), const char *what, const char *noun);
void *arthip_malloc (size_t bytes);
void  arthip_free (void *p);
int   arthip_h2d (void *dst, const void *src, size_t bytes, void *stream);
int   arthip_d2h (void *dst, const void *src, size_t bytes, void *stream);
int   arthip_d2d (void *dst, const void *src, size_t bytes, void *stream);
int   arthip_zero (void *dst, size_t bytes, void *stream);
int   arthip_sync (void *stream);
const char *arthip_last_error (void);
void arthip_set_last_error (const char *text);
void *arthip_event_create (void);
void  arthip_event_destroy (void *ev);
int   arthip_event_record (void *ev, void *stream);
float arthip_event_elapsed_ms (void *start, void *stop);   /* synchronises on `stop` */

/* ---- sinc_fir.hip ---- */
/* returns the kernel actually used (ART_KERNEL_*), <0 on launch failure */
int arthip_fir (const ArtFirArgs *a, const ArtSegTable *segs, int kernel_pref, void *stream);
/* What a call's launches need, asked once per call before its buffers exist (the buffer pointers of `call` are not looked at; rows_cache is: the
 * cut-invariant policy's launches shorter than a period are the matrix path's only with kept rows).  `call` = the call's ArtFirArgs, `first` = its
 * first segment table (the first ART_MAX_SEGS segments of a longer call), `outputs` = its output frames. */
typedef struct {
    int matrix;                          /* the call's launches may take the matrix-core path: provision the buffers below (0: none, all sizes 0) */
    int one_launch;                      /* a call of more than ART_MAX_SEGS segments may be ONE launch on its first table (segs_truncated): it runs on a
                                          * streaming matrix-core kernel, which follows the lattice of the launch's first period, not the table */
    size_t scratch_bytes;                /* ArtFirArgs.scratch (and the counters fix_count / fix_list) */
    size_t planes_bytes;                 /* ArtFirArgs.planes: the fixed-point kernel's digit planes (0: the call is the f32 kernels') */
    size_t rows_bytes;                   /* ArtFirArgs.rows: the matrix kernels' rows kept across calls (0: none) */
    size_t split_bytes;                  /* ArtFirArgs.split: the K-split kernel's counters and partial sums (0: unsplit) */
    size_t pad_bytes;                    /* ArtFirArgs.pad: the channel groups' padded copies (0: the stream is of a compiled width) */
} ArtFirNeeds;
void arthip_fir_needs (const ArtFirArgs *call, const ArtSegTable *first, unsigned int outputs, int kernel_pref, ArtFirNeeds *out);
/* the fixed-point kernel's rows across the calls of a context (ArtFirArgs.rows / rows_cache): size of the host block that describes the device
 * buffer (zeroed by the owner), forgetting what the buffer held (it was replaced), releasing what the host block owns */
size_t arthip_fir_rows_cache_bytes (void);
void   arthip_fir_rows_cache_reset (void *cache);
void   arthip_fir_rows_cache_free (void *cache);
/* n independent general-kernel calls (default / precise mode) in one launch per kernel variant; d_table = device scratch of
 * n * arthip_fir_batch_item_bytes () bytes (reused call after call: stream order protects it); asynchronous like arthip_fir */
size_t arthip_fir_batch_item_bytes (void);
int arthip_fir_batch_max_segments (void);                /* ring-epoch segments a batched call may have */
int arthip_fir_batch (const ArtFirArgs *a, const ArtSegTable *segs, int n, void *d_table, void *stream);
/* may this general-kernel call be an item of arthip_fir_batch?  (its one-output tile's span must fit the launches' shared LDS budget: a ratio
 * below that is the single call's — more LDS for itself, or the strict kernel) */
int arthip_fir_batch_accepts (const ArtFirArgs *call);
/* n independent calls of the f32 streaming matrix-core kernel in one launch per shape (4-byte build; the 8-byte build plans none).
 * arthip_fir_group_plan: `a` / `segs` as arthip_fir would get them (buffers provisioned, roll_dst set, no timing events) — would that call be ONE
 * regular, un-split launch of that kernel on rows kept across calls whose set is built?  1: *out is that launch, nothing enqueued, and the
 * context's host-side rows cache is as the single launch's own look-ups leave it; 0: the call is made as it stands (arthip_fir), as if never asked.
 * Calls of one shape (arthip_fir_group_same_class) may share a launch: the caller numbers the classes it wants launched 0 .. in `cls` and hands
 * them to arthip_fir_group with device memory of arthip_fir_group_table_bytes (n) bytes (reused call after call: stream order protects it).
 * Returns 0, or -1 with nothing enqueued; the history rolls ride along (every call as ART_KERNEL_MFMA | ART_FIR_ROLLED where roll_dst is set). */
typedef struct {
    ArtFirArgs a;                        /* the launch, anchored on the stream's canonical period */
    int cls;                             /* the caller's: the launch class of this call */
    int fixup;                           /* the nearest-filter pass-through pass follows the launch */
    union { char bytes [160]; double align; } geom;     /* the launch's tile geometry (fir_matrix.hip) */
} ArtFirGroupCall;
int arthip_fir_group_plan (const ArtFirArgs *a, const ArtSegTable *segs, int kernel_pref, ArtFirGroupCall *out);
int arthip_fir_group_same_class (const ArtFirGroupCall *x, const ArtFirGroupCall *y);
size_t arthip_fir_group_table_bytes (int n);
int arthip_fir_group (const ArtFirGroupCall *calls, int n, void *d_table, void *stream);
/* Consecutive blocks of ONE stream as one general-kernel launch (resampleProcessScheduleInterleavedDevice).  The run's linear space is
 * (history ++ run input); a block is the single call it replaces, moved in_off frames along it. */
typedef struct {
    double ratio;                        /* the block's effective ratio */
    unsigned int out_off, outputs;       /* its first output frame within the run's output, and its output frames (> 0) */
    int in_off, in_end;                  /* its first input frame within the run's input, and the end of what it may read (in_off + input used) */
    int lin_floor;                       /* run-linear index below which its reads are silence (>= in_off) */
    int seg_begin, seg_end;              /* its segments in the run's segment array (first_output block-relative, lin_base the block's own) */
    unsigned int first_tile;             /* filled by arthip_fir_schedule */
    int pad;
} ArtSchedBlock;
typedef struct { unsigned int first; int lin_base; double base; } ArtSchedSeg;
/* may this block (its planned segments, outputs) be part of a run?  (its tile's span must fit the LDS, and a tile may touch only as many
 * segments as the kernel rebuilds) */
int arthip_fir_schedule_accepts (const ArtFirArgs *block, const ArtamdSegment *segs, int nseg, unsigned int outputs);
/* One launch over the run's blocks.  `run` = the run's FIR arguments (hist, in = the run's input, out = the run's output, in_frames and
 * roll_appended = the run's input frames, roll_dst, timing events); d_table: device memory of arthip_fir_schedule_bytes bytes (reused run
 * after run: stream order protects it).  Returns ART_KERNEL_GENERAL | ART_FIR_ROLLED, or -1 with nothing enqueued. */
size_t arthip_fir_schedule_bytes (int nblocks, int nsegs);
int arthip_fir_schedule (const ArtFirArgs *run, ArtSchedBlock *blocks, int nblocks, const ArtSchedSeg *segs, int nsegs, void *d_table, void *stream);
/* The runs of MANY streams as one launch per kernel variant (resampleProcessScheduleBatch*Device; fir_general_schedule_batch_kernel).  An item is
 * what arthip_fir_schedule would get for its stream (nblocks > 0; no timing events), each keeps the tile of its own launch; the history rolls
 * ride along.  One upload carries every item, block and segment: d_table is device memory of arthip_fir_schedule_batch_bytes bytes (reused call
 * after call: stream order protects it).  Returns the number of launches enqueued, every item's `launched` 1 — or -1: a launch failed (or the
 * ARTAMD_TEST_FAIL_FIR hook, which counts one per call of this function, before anything is enqueued) and `launched` says whose run is on the
 * stream all the same (all 0 where nothing was enqueued). */
typedef struct {
    ArtFirArgs run;
    const ArtSchedBlock *blocks; int nblocks;
    const ArtSchedSeg *segs; int nsegs;
    int launched;
} ArtSchedItem;
size_t arthip_fir_schedule_batch_bytes (int nitems, int nblocks, int nsegs);
int arthip_fir_schedule_batch (ArtSchedItem *items, int n, void *d_table, void *stream);
/* ---- fir_adjoint.hip: the transpose of the whole-clip interpolator (resampleAdjointClipsPlanarDevice) ----
 * An item is one clip: gx [0, in_frames) of every channel = the sum over the clip's outputs n, ascending, of weight (n, j) * gy [n].  The outputs
 * are those of two planned calls from a fresh context — phase 0 the process call, phase 1 the flush — whose linear spaces hold input frame j at
 * H + j and at H + j - in_frames (the history after the roll); the flush reads nothing below its lin_floor.  Each phase's segments are
 * seg_count [p] entries from seg_first [p] on in the call's segment list. */
typedef struct {
    const art_s *bank;                   /* device, (F+1) x T */
    const art_s *gy;                     /* gradient of the outputs: gy_frames frames, the rest of the clip's outputs count as zero */
    art_s *gx;                           /* gradient of the inputs: in_frames frames are SET */
    long gy_pitch, gx_pitch;             /* samples between planes; 0: that side interleaved */
    double ratio;                        /* the effective ratio (locate: a.ratio) */
    unsigned int outputs [2];            /* output frames of the two phases */
    unsigned int gy_frames;
    unsigned int tile0;                  /* first tile of the item in its launch (filled by arthip_fir_adjoint) */
    int seg_first [2], seg_count [2];
    int lin_floor;                       /* the flush's (INT_MIN: none) */
    int in_frames, C, T, F;              /* in_frames > 0 */
    int interpolate, lowpass;
} ArtAdjItem;
size_t arthip_fir_adjoint_bytes (int nitems, int nsegs);
/* One launch per kernel variant present (channel-group width x interpolating or not) over the items' tiles of input frames.  The items (reordered
 * by variant) and the nsegs segments go to d_table (device memory of arthip_fir_adjoint_bytes bytes, reused call after call: stream order protects
 * it) in one upload.  Returns the number of launches enqueued, or -1 (a launch failed; nothing enqueued where the upload could not be made). */
int arthip_fir_adjoint (const ArtAdjItem *items, int n, const ArtamdSegment *segs, int nsegs, void *d_table, void *stream);
/* ... of clips made block by block (resampleAdjointScheduleClipsPlanarDevice; fir_adjoint_blocks_kernel): any number of phases per clip, one planned
 * call each — the blocks' process calls in turn, each at its own ratio, then the flush — in a phase table beside the items.  Phase k's linear
 * space holds input frame j at H + j - start; it reads no frame at or past `end` and nothing below `floor`.  start and end do not decrease
 * from one phase of a clip to the next. */
typedef struct {
    double ratio;                        /* the effective ratio of the phase's call (locate: a.ratio) */
    unsigned int outputs;                /* output frames of the phase */
    unsigned int first_output;           /* its first output among the clip's */
    int seg_first, seg_count;            /* its segments in the call's segment list */
    int start, end;                      /* input frames of the clip before the phase's call, and with it (the flush: in_frames both) */
    int floor;                           /* max (0, the call's lin_floor) */
    int pad;
} ArtAdjPhase;
typedef struct {
    const art_s *bank;                   /* device, (F+1) x T */
    const art_s *gy;                     /* gradient of the outputs: gy_frames frames, the rest of the clip's outputs count as zero */
    art_s *gx;                           /* gradient of the inputs: in_frames frames are SET */
    long gy_pitch, gx_pitch;             /* samples between planes; 0: that side interleaved */
    unsigned int gy_frames;
    unsigned int tile0;                  /* first tile of the item in its launch (filled by arthip_fir_adjoint_blocks) */
    int phase_first, phase_count;        /* the clip's phases in the call's phase table (>= 2; the last is the flush) */
    int in_frames, C, T, F;              /* in_frames > 0 */
    int interpolate, lowpass;
} ArtAdjBlocksItem;
size_t arthip_fir_adjoint_blocks_bytes (int nitems, int nphases, int nsegs);
/* as arthip_fir_adjoint: one launch per kernel variant present; items, phases and segments go to d_table in one upload */
int arthip_fir_adjoint_blocks (const ArtAdjBlocksItem *items, int n, const ArtAdjPhase *phases, int nphases, const ArtamdSegment *segs, int nsegs,
                               void *d_table, void *stream);
/* ---- fir_rate_grad.hip: the gradient of such clips with respect to their blocks' ratios (resampleRateGradientScheduleClipsPlanarDevice) ----
 * An item is one clip on an interpolating context: its phases are the blocks adjoint's (the same ArtAdjPhase table, the last the flush), its
 * samples are read where that kernel writes gx.  The first launch's tasks are tiles of ART_RATE_TILE consecutive outputs of one phase; a
 * phase without outputs has none. */
#define ART_RATE_TILE 256
typedef struct {
    const art_s *bank;                   /* device, (F+1) x T */
    const art_s *x;                      /* the clip's samples: in_frames frames */
    const art_s *gy;                     /* gradient of the outputs: gy_frames frames, the rest of the clip's outputs count as zero */
    double *grad;                        /* phase_count - 1 doubles are SET: dL/dr of every block */
    long x_pitch, gy_pitch;              /* samples between planes; 0: that side interleaved */
    unsigned int gy_frames;
    int phase_first, phase_count;        /* the clip's phases in the call's phase table (>= 2; the last is the flush) */
    int in_frames, C, T, F;              /* in_frames >= 0 (an empty clip: gy_frames 0, a zero for its block) */
    int pad;
} ArtRateItem;
size_t arthip_fir_rate_grad_bytes (int nitems, int nphases, int nsegs, unsigned long tiles);
/* ceil (outputs / ART_RATE_TILE) summed over the phases: what the call's scratch holds a pair of doubles for */
unsigned long arthip_fir_rate_grad_tiles (const ArtAdjPhase *phases, int nphases);
/* Two launches — the tiles' partial sums, then one wave per clip (one launch where no phase has an output).  Items, phases, the phases' first
 * tasks and the segments go to d_table (device memory of arthip_fir_rate_grad_bytes bytes, reused call after call: stream order protects it) in
 * one upload; the partials follow them there.  Returns the number of launches enqueued, or -1 (a launch failed; nothing enqueued where the
 * upload could not be made). */
int arthip_fir_rate_grad (const ArtRateItem *items, int n, const ArtAdjPhase *phases, int nphases, const ArtamdSegment *segs, int nsegs,
                          void *d_table, void *stream);
/* ---- fir_sample.hip: whole clips at a position curve in device memory (resampleSample*ClipsPlanarDevice, resampleSampleBand*ClipsPlanarDevice) ----
 * An item is one clip and its curve of `gy_frames` positions (doubles, in input frames; p = 0 is centred on frame 0).  One struct serves the
 * three launches of both families: the forward reads in and writes out = y; the adjoint reads gy and writes out = gx; the slope reads in and
 * gy and writes gp — on the banded entries gp, gl or both, whichever is not NULL (the same in every item of a launch: the entry's lists).
 * The unbanded entries' item has its context's bank as rung 0, rungs = 1 and no levels; a banded item holds a LADDER of `rungs` banks of one
 * shape (interpolating contexts only) and a curve of gy_frames levels beside the positions.
 * The forward's and the slope's tasks are tiles of ART_SAMPLE_TILE consecutive outputs, the adjoint's tiles of ART_SAMPLE_TILE consecutive
 * input frames times the item's channel groups; an item is in a launch only if it has a task. */
#define ART_SAMPLE_TILE 256
#define ART_BAND_RUNGS 8
enum { ART_SAMPLE_FORWARD, ART_SAMPLE_ADJOINT, ART_SAMPLE_SLOPE };
typedef struct {
    const art_s *bank [ART_BAND_RUNGS];  /* device, (F+1) x T each; [0, rungs) */
    const double *pos, *level;           /* the curve: gy_frames doubles; the levels beside it (NULL: the unbanded entries) */
    const art_s *in;                     /* the clip's samples: in_frames frames (forward, slope) */
    const art_s *gy;                     /* gradient of the outputs: gy_frames frames (adjoint, slope) */
    art_s *out;                          /* forward: y, gy_frames frames are SET; adjoint: gx, in_frames frames are SET */
    double *gp, *gl;                     /* slope: gy_frames doubles are SET in each that is there */
    long in_pitch, gy_pitch, out_pitch;  /* samples between planes; 0: that side interleaved */
    unsigned int gy_frames;              /* M: the curve's length = the clip's outputs */
    unsigned int task0;                  /* first task of the item in its launch (filled by arthip_fir_sample) */
    int in_frames, C, T, F;
    int rungs, interpolate, lowpass, pad;
} ArtSampleItem;
/* tasks of one item in launch `what` (0: the item is no part of it) */
unsigned long arthip_fir_sample_tasks (const ArtSampleItem *it, int what);
size_t arthip_fir_sample_bytes (int nitems);
/* ONE launch of kernel `what` — `band`: of the banded family — over the items (every one with a task at least; their tasks' sum fits an int).
 * The items go to d_table (device memory of arthip_fir_sample_bytes bytes, reused call after call: stream order protects it) in one upload.
 * Returns 1, 0 for n <= 0, or -1 (the launch failed; nothing enqueued where the upload could not be made). */
int arthip_fir_sample (const ArtSampleItem *items, int n, int what, int band, void *d_table, void *stream);
/* the upkeep every launch of a rational-ratio stream does for the rows kept across calls (arthip_fir calls it itself) */
void arthip_fir_rows_touch (const ArtFirArgs *a, const ArtSegTable *segs);
/* new_hist[H][C] = last H frames of (hist ++ in[0..appended)); in may be NULL => zeros appended */
int arthip_roll_history (art_s *new_hist, const art_s *hist, const art_s *in, long in_pitch, int appended, int H, int C, void *stream);
int arthip_interleave (art_s *dst, const art_s *src_planar, long pitch, int frames, int C, void *stream);
int arthip_deinterleave (art_s *dst_planar, long pitch, const art_s *src, int frames, int C, void *stream);

/* ---- layout_kernels.hip: the same two copies for many buffers in one launch (transpose_group_kernel) ---- */
typedef struct {
    art_s *planes;                       /* the planar side: channel c at planes + c * pitch */
    art_s *frames;                       /* the interleaved side: [frame][C] */
    long pitch;                          /* samples between planes (>= count; any alignment) */
    long task0;                          /* first task of this item in the launch's flattened task space (filled by the launch) */
    int count, C;                        /* frames to move (> 0), channels */
    int tile, pad;                       /* frames per task (filled by the launch) */
} ArtLayoutItem;
/* uploads the n items through the shared pinned staging into d_table (device memory of n items, reused call after call: stream order protects
 * it) and moves every item in one launch on `stream`: planes -> frames, or (to_planar) frames -> planes; 0, or -1 (nothing launched) */
int arthip_transpose_group (ArtLayoutItem *items, int n, int to_planar, void *d_table, void *stream);

/* ---- extrapolate_kernels.hip: LPC end-point extrapolation, one workgroup per run ----
 * A run's known samples, oldest first, are n[0] samples at src[0] + j * stride[0] followed by n[1] at src[1] + j * stride[1]
 * (n[0] + n[1] in 8 .. ARTAMD_EXTRAPOLATE_MAX_KNOWN).  backward == 0: the `extras` samples that continue past the newest
 * (reference extrapolate_forward); != 0: the `extras` samples that precede the oldest, nearest first (extrapolate_reverse).
 * Sample i goes to out + i * out_stride (a negative stride walks back through an interleaved history). */
typedef struct {
    const art_s *src [2];
    long stride [2];
    int n [2];
    art_s *out;
    long out_stride;
    int extras, backward;
} ArtExtrapRun;
/* uploads the n runs (table of the calling thread, device memory kept across calls) and launches them on `stream`; 0, or -1 */
int arthip_extrapolate (const ArtExtrapRun *runs, int n, void *stream);

/* ---- pcm_kernels.hip ---- */
typedef struct {
    int C, bits, bytes, dither_type, dither_on, shaping_on;
    int shaping_order;                   /* order of the error-feedback filter (same for every channel) */
    art_s scale;
    art_s *feedback;                     /* device [C] */
    uint32_t *gens;                      /* device [C] */
    uint32_t *gens_next;                 /* device [C]: where the fully parallel kernel leaves the generator state */
    Biquad *shapers;                     /* device [C] */
    unsigned long long *clipped;         /* device counter */
} ArtDecArgs;
/* returns 1 when the generator state was written to a->gens_next (caller swaps), 0 otherwise, <0 on error */
int arthip_decimate (const ArtDecArgs *a, const art_s *d_in, int frames, unsigned char *d_out, void *stream);
/* THE planar call: arthip_decimate on planes, channel c of the input at d_in + c * in_pitch (samples), of the output at
 * d_out + c * out_pitch (bytes); a pitch of 0: that side is interleaved (both 0: arthip_decimate).  The same kernel as the
 * interleaved call would run, and the same return values */
int arthip_decimate_pitched (const ArtDecArgs *a, const art_s *d_in, long in_pitch, int frames, unsigned char *d_out, long out_pitch, void *stream);
/* NOT the planar call, whatever its name says: always the one-lane kernel (decimate_kernel), whatever the frame count — the
 * host-pointer planar entry's (decimateProcessLE), whose generator state must stay where it is.  Returns 0, or <0 on error */
int arthip_decimate_planar (const ArtDecArgs *a, const art_s *d_in, long in_pitch, int frames, unsigned char *d_out, long out_pitch, void *stream);
/* Many contexts' calls, one launch per class (decimateProcessBatchInterleavedLEDevice).  The host builds one table per call (the
 * classes' item arrays one after another, each 16-byte aligned), uploads it once and launches every class from its slice. */
typedef struct {                         /* one channel of one context: a lane of the serial wave (noise shaping, or short calls) */
    const art_s *in;                     /* the lane's first input sample (interleaved: input + channel, planar: its plane); frame f at in [f * stride] */
    unsigned char *out;                  /* the lane's first output byte (interleaved: output + channel * bytes, planar: its plane); frame f at out [f * out_stride * bytes] */
    art_s *feedback;                     /* &feedback [channel] */
    uint32_t *gen;                       /* &gens [channel] (NULL without dither) */
    Biquad *shaper;                      /* &shapers [channel] (NULL without noise shaping) */
    unsigned long long *clipped;         /* the context's counter */
    art_s scale;
    int stride, frames, bits, bytes, dither_type;     /* frames 0: an empty lane (padding of the last workgroup) */
    int out_stride;                      /* stride / out_stride: frames between the lane's samples on either side — the channel count, or 1 on a planar side */
} ArtDecLane;
typedef struct {                         /* one context of a time-parallel launch (no noise shaping, >= 64 frames) */
    const art_s *in;
    unsigned char *out;
    art_s *feedback;
    uint32_t *gens, *gens_next;          /* the generator state is read from gens and left in gens_next (the host swaps them) */
    unsigned long long *clipped;
    long task0;                          /* first (channel, segment) task of this context in the launch's flattened task space */
    art_s scale;
    int C, frames, bits, bytes, dither_type;
    long in_pitch, out_pitch;            /* samples / bytes between the planes of that side; 0: that side is interleaved */
} ArtDecTask;
/* The clips entry's records (decimateProcessClipsPlanarLEDevice): the batch entry's, plus where the first state is read from (the
 * image decimateInit left, with fromStart; else the live state, which is always what is written) and the item's own clip count.
 * Record types of their own and kernels of their own (over the same bodies): the batch entry's kernels and tables stay what they were. */
typedef struct {
    ArtDecLane lane;
    const art_s *feedback_from;          /* what lane.feedback / lane.gen / lane.shaper start from */
    const uint32_t *gen_from;
    const Biquad *shaper_from;
    unsigned long long *item_clipped;    /* &d_clipCounts [item], or NULL: this call's clipped samples of the lane are added here too */
} ArtDecClipLane;
typedef struct {
    ArtDecTask task;                     /* (task.feedback and task.gens are only read: with fromStart they point into the image) */
    unsigned long long *item_clipped;
    long task0;                          /* task.task0 again, where the kernels' search over the items looks for it */
} ArtDecClipTask;
typedef struct {                         /* a class's slice of a batch call's table (16-byte aligned) */
    int count;                           /* items; in a serial class, lanes (a multiple of `lanes`: empty lanes pad the last workgroup) */
    int lanes;                           /* serial classes: lanes per workgroup */
    size_t offset;                       /* of the class's items in the table */
} ArtBatchSlice;
typedef struct {
    int serial;                          /* 1: ArtDecLane items (lanes per workgroup slice.lanes), 0: ArtDecTask items */
    int order, dither;                   /* the shaper order (0: none) and whether dither is on: every item of the class shares them */
    long tasks;                          /* time-parallel: total tasks */
    int pitched;                         /* an item of the class has a planar side: the kernel's PITCHED instantiation */
    int clips;                           /* the items are the clips entry's records (ArtDecClipLane / ArtDecClipTask) and run its kernels */
    ArtBatchSlice slice;
} ArtDecClass;
#define ART_DEC_SEG 32                   /* frames of one channel per task of the time-parallel kernels (even: generator pairs) */
/* the lane count per workgroup the batch gives a serial class of `lanes` lanes in all */
int arthip_decimate_batch_lanes (int lanes);
/* one launch of one class from its slice of the uploaded table; 0 or -1 (nothing of it ran) */
int arthip_decimate_batch_launch (const ArtDecClass *cls, const void *d_table, void *stream);
/* decimateProcessBatchInterleavedLEDevice with a fixed lane count per workgroup for every serial class (lanes > 0; 0: the rule
 * of arthip_decimate_batch_lanes): the measurements behind that rule (tools/bench_decimate_batch.py) — pcm_host.c */
int artamd_decimate_batch (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const int *numInputFrames,
                           unsigned char *const *d_outputs, int lanes);
/* ... and decimateProcessBatchPlanarLEDevice likewise: the one body of both layouts (NULL pitch arrays: artamd_decimate_batch) */
int artamd_decimate_batch_planar (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                  const int *numInputFrames, unsigned char *const *d_outputs, const long *outputPitches, int lanes);
/* ... and decimateProcessClipsPlanarLEDevice: the same body once more, with the clips entry's records when fromStart or d_clipCounts ask for them */
int artamd_decimate_clips_planar (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                  const int *numInputFrames, unsigned char *const *d_outputs, const long *outputPitches, int lanes,
                                  int fromStart, unsigned long long *d_clipCounts);
int arthip_biquad_chain (Biquad *d_sections, int C, int S, art_s *d_buf, int frames, int stride, void *stream);
/* Many banks' calls, one launch per section count (biquadBankApplyBatchInterleavedDevice).  A lane is one channel of one bank;
 * each class's lanes are one slice of the call's table (16-byte aligned), uploaded with arthip_table_upload. */
typedef struct {
    Biquad *sections;                    /* the bank's d_sections + channel * S */
    art_s *buf;                          /* the bank's buffer + channel; frame f at buf [f * stride], in place */
    int stride, frames;                  /* frames 0: an empty lane (padding of the last workgroup) */
} ArtBqLane;
typedef struct {
    int S;                               /* sections per channel: every lane of the class has S */
    ArtBatchSlice slice;
} ArtBqClass;
/* the lane count per workgroup the batch gives a class of `lanes` lanes in all */
int arthip_biquad_batch_lanes (int lanes);
/* one launch of one class from its slice of the uploaded table; 0 or -1 (nothing of it ran) */
int arthip_biquad_batch_launch (const ArtBqClass *cls, const void *d_table, void *stream);
/* biquadBankApplyBatchInterleavedDevice with a fixed lane count per workgroup (lanes > 0; 0: arthip_biquad_batch_lanes) and a
 * fixed bound on the frames of a gathered time-parallel call (serialMax >= 0; < 0: the library's): the measurements behind both
 * (tools/bench_biquad_batch.py) — pcm_host.c */
int artamd_biquad_batch (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const int *numFrames, int lanes, int serialMax);
/* ... and biquadBankApplyBatchPlanarDevice likewise: the one body of both layouts (NULL pitches: artamd_biquad_batch).  A planar
 * item's lane is a plane: buf = the item's buffer + channel * pitch, stride 1 */
int artamd_biquad_batch_planar (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const long *pitches, const int *numFrames,
                                int lanes, int serialMax);
int artamd_biquad_batch_serial_max (void);                              /* the library's bound (BQ_BATCH_SERIAL_MAX) */
/* every section has order 2, S = 1 or 2, interleaved frames: hand-scheduled kernel */
int arthip_biquad_order2 (Biquad *d_sections, int C, int S, art_s *d_buf, int frames, int stride, void *stream);   /* stride >= C: values between frames */
/* bit-exact cascade, parallel over time (speculative chunks + exact verification, pcm_kernels.hip): d_in -> d_out, distinct
 * buffers; L = chunk length, W = warm-up frames per section; d_states: arthip_biquad_spec_scratch () bytes of scratch */
size_t arthip_biquad_spec_scratch (int C, int S, int frames, int L);
int arthip_biquad_spec_arm (int *d_first_bad, int C, void *stream);      /* once per scratch: C ints the calls keep at "no mismatch" */
int arthip_biquad_spec (Biquad *d_sections, int C, int S, const art_s *d_in, int in_stride, art_s *d_out, int out_stride, int frames,
                        int L, int W, void *d_states, int *d_first_bad, unsigned int *d_repairs, void *stream);
/* the same over planes: channel c's frames are consecutive from d_in + c * in_pitch and go to d_out + c * out_pitch (pitches in
 * samples; distinct buffers).  A lane moves its run 16 bytes at a time, cut at the 16-byte boundaries of the run's own address;
 * its stores are whole too where the two planes' addresses agree modulo 16 */
int arthip_biquad_spec_planar (Biquad *d_sections, int C, int S, const art_s *d_in, long in_pitch, art_s *d_out, long out_pitch, int frames,
                               int L, int W, void *d_states, int *d_first_bad, unsigned int *d_repairs, void *stream);
/* Many banks' time-parallel calls in shared launches (biquadBankApplyClipsPlanarDevice).  An item is one bank's call, with the
 * chunk length, chunk count and warm-up its single call would use; a class is the items of one section count and one layout. */
typedef struct {
    const Biquad *from;                  /* coefficients and carried-in state: the bank's d_sections, or d_sections0 (fromStart) */
    Biquad *sections;                    /* the bank's d_sections: the final state goes here */
    const art_s *in;                     /* the call's frames, set aside in the shared scratch */
    art_s *out;                          /* the caller's buffer */
    long in_stride, out_stride;          /* a planar class: samples between planes; an interleaved one: values between frames */
    void *states;                        /* arthip_biquad_spec_scratch () bytes: starts, ends, flags, as the single call lays them out */
    int *first_bad;                      /* the bank's own */
    unsigned int *repairs;               /* the bank's own */
    long task0;                          /* first (chunk, channel) task of the item in the class's flattened task space */
    int chan0;                           /* first channel of the item among the class's channels (the commit launch's threads) */
    int C, K, L, W, frames;
} ArtBqClip;
typedef struct {
    int S, planar;
    int count, channels;                 /* items; channels of all of them */
    long tasks;                          /* (chunk, channel) tasks of all of them */
    size_t offset;                       /* of the class's items in the table (16-byte aligned) */
} ArtBqClipClass;
/* spec, check and commit launch of one class; 0 or -1 */
int arthip_biquad_clips_launch (const ArtBqClipClass *cls, const void *d_table, void *stream);
/* Many whole clips OUT OF PLACE from the banks' first state, forwards or with time reversed (biquadBankFilterClipsPlanarDevice).
 * The time-parallel items are ArtBqClip records in ArtBqClipClass classes again, with these differences: `from` is the bank's
 * d_sections0 and `sections` is NULL (nothing is stored back), `in` is the caller's input where it lies, `first_bad` points behind
 * the item's own `states` (C ints, armed by the spec launch) and `repairs` is the leading bank's counter.  Reversed: frame n of
 * the recurrence lives at address frames - 1 - n on both sides.  Spec, check and commit launch of one class; 0 or -1 */
int arthip_biquad_filter_clips_launch (const ArtBqClipClass *cls, const void *d_table, int reversed, void *stream);
/* ... and their serial route: a lane is one channel of one item, read at `in` and written at `out` */
typedef struct {
    const Biquad *sections;              /* the bank's d_sections0 + channel * S: only read */
    const art_s *in;                     /* the item's input + channel (or plane); frame f at in [f * in_stride] */
    art_s *out;                          /* likewise */
    int in_stride, out_stride, frames;   /* frames 0: an empty lane (padding of the last workgroup) */
} ArtBqFilterLane;
int arthip_biquad_filter_batch_launch (const ArtBqClass *cls, const void *d_table, int reversed, void *stream);
/* biquadBankFilterClipsPlanarDevice with a byte bound per round (roundBytes > 0; else the library's): the tests' three rounds — pcm_host.c */
int artamd_biquad_filter_clips_planar (BiquadBank *const *banks, int n, const artsample_t *const *d_ins, const long *in_pitches,
                                       artsample_t *const *d_outs, const long *out_pitches, const int *numFrames, int reversed, long roundBytes);
typedef struct {                         /* one strided copy of a grouped copy launch; everything in 4-byte words */
    const unsigned int *src;
    unsigned int *dst;
    long src_pitch, dst_pitch;           /* between row starts */
    long width, rows;                    /* words per row */
    long groups;                         /* tasks per row: (width + 3) / 4 + 1 (16-byte groups counted from the boundary before the row) */
    long task0;                          /* first task of the item: the sum of rows * groups of the items before it */
} ArtCopyRows;
int arthip_copy_rows_launch (const void *d_items, int n, long tasks, void *stream);
typedef struct {                         /* one run of a grouped zeroing launch (layout_kernels.hip): `words` 4-byte words from `ptr` on */
    unsigned int *ptr;                   /* 4-byte aligned */
    long words;
    long task0;                          /* first task of the item: a task clears up to 4 words, (words + 3) / 4 + 1 tasks per item */
} ArtZeroRun;
/* every run cleared in one launch: fills the items' task0, uploads them to d_table (n items of device memory) and launches; 0 or -1 */
int arthip_zero_runs (ArtZeroRun *items, int n, void *d_table, void *stream);
/* biquadBankApplyClipsPlanarDevice with its own bound on the bytes set aside per round (roundBytes > 0; else the library's,
 * BQ_CLIPS_ROUND_BYTES): how the tests make a small batch take several rounds — pcm_host.c */
int artamd_biquad_clips_planar (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const long *pitches, const int *numFrames,
                                int fromStart, long roundBytes);
/* ---- time stretcher (stretch_kernels.hip) ---- */
typedef struct {
    art_s *ring [2][2];                  /* [stage][ping-pong] input rings, `room` values each */
    art_s *between;                      /* hand-over buffer stage 1 -> stage 2 (cascaded pair) */
    art_s *total, *score;                /* search scratch: longest + 4 values each */
    void *state;                         /* device: { int mark, fill, cur, pad; double drift; } per stage */
    int channels, room, lo, hi, quick, paired;
} ArtStretchArgs;
/* one stretchProcess (flush == 0) or stretchFlush (flush != 0) call; *d_result receives the frames written */
int arthip_stretch_call (const ArtStretchArgs *h, const art_s *d_in, int frames, art_s *d_out, double ratio, int flush,
                         int *d_result, void *stream);

/* the same call on n independent streams in ONE launch (one workgroup per stream): d_items / d_done in device memory */
typedef struct { int mark, fill, cur, pad; double drift; } ArtStretchState;          /* per stage; layout of stretch_kernels.hip */
typedef struct { ArtStretchArgs args; const art_s *in; art_s *out; double ratio; int frames, flush; } ArtStretchItem;
typedef struct { int made, pad; ArtStretchState state [2]; } ArtStretchDone;
int arthip_stretch_batch (const ArtStretchItem *d_items, ArtStretchDone *d_done, int n, void *stream);
/* whole clips, one workgroup each in ONE launch: from the state stretchInit leaves where from_start, the process call (frames > 0),
 * then the flushes until one gives nothing, written behind one another.  Channel c of the input is at in + c * in_pitch samples, of
 * the output at out + c * out_pitch (0: that side interleaved).  No bounds checks: the caller has made sure `out` holds it all */
typedef struct { ArtStretchArgs args; const art_s *in; art_s *out; long in_pitch, out_pitch; double ratio; int frames, from_start; } ArtStretchClip;
int arthip_stretch_clips (const ArtStretchClip *d_items, ArtStretchDone *d_done, int n, void *stream);
/* the same launch from a fresh start (from_start is taken as set) with the splice log (art_hip.h) written: item i's stages write their
 * segments to d_logs [i].seg [0 / 1] (the second unused for a single stage) and their number to d_counts [2 i], [2 i + 1].  No bounds
 * checks on the logs either */
typedef struct { ArtamdStretchSegment *seg [2]; } ArtStretchLogs;
int arthip_stretch_clips_logged (const ArtStretchClip *d_items, ArtStretchDone *d_done, const ArtStretchLogs *d_logs, int *d_counts, int n, void *stream);

/* ---- transpose of a logged stage (stretch_adjoint.hip) ---- */
/* One stage of one clip: gx [v] for the values v < gx_values of the stage's input stream from the segments of `log`, terms at outputs
 * o >= gy_values dropped.  Values are addressed as the forward addresses them: value v is channel v % channels of frame v / channels, at
 * base + channel * pitch + frame (pitch != 0) or base + v (pitch 0: interleaved).  `mid` != NULL (a cascaded pair): the count of the
 * intermediate stream — gx_values of its second stage (mid_is_gx), gy_values of its first — is read on the device: the end of the last
 * of the mid_count segments of stage 1's log (0 for none); the host's figure is then only the bound the tiles were laid out for.
 * A segment reads nothing below from - back and nothing at or above from + ahead (values): a longest period, the ring. */
typedef struct {
    const ArtamdStretchSegment *log, *mid;
    const art_s *gy; art_s *gx;
    long gy_pitch, gx_pitch;
    int count, mid_count, mid_is_gx;
    int gy_values, gx_values;
    int channels, back, ahead;
    unsigned int tile0;                  /* first workgroup of the item in its launch (filled by arthip_stretch_adjoint) */
    int pad;
} ArtStretchAdjItem;
/* uploads the n items to d_table (n items of device memory) and launches one workgroup per tile of each; 0 or -1 */
int arthip_stretch_adjoint (ArtStretchAdjItem *items, int n, void *d_table, void *stream);

/* a failure of an entry point that cannot return one (the reference's ABI has no error codes): printed, counted (artamdErrorCount /
 * artamdLastError), fatal under ARTAMD_ABORT_ON_ERROR=1 — pcm_host.c */
void artamd_note_failure (const char *what);

int arthip_ingest (const unsigned char *d_in, art_s gain_factor, int bits, int bytes, int stride, art_s *d_out, int n, void *stream);
/* Many buffers' ingest in one launch (floatIntegersBatchLEDevice).  A task is a run of ART_INGEST_RUN consecutive samples of one
 * item (16 bytes of output); an item's runs start `head` samples before its first sample, so that every whole run of an output
 * aligned to its sample size is 16-byte aligned. */
#define ART_INGEST_RUN ((int)(16 / sizeof (art_s)))
typedef struct {
    const unsigned char *in;
    art_s *out;
    long task0;                          /* first task of this item in the launch's flattened task space */
    art_s gain_factor;                   /* ingest_gain (gain, bits): the single call's factor */
    int bits, bytes, stride, count, head;     /* count > 0 samples; 0 <= head < ART_INGEST_RUN */
} ArtIngestItem;
/* uploads the n items (table of the calling thread, device memory kept across calls) through the shared pinned staging and launches
 * ingest_batch_kernel over `tasks` tasks on `stream`; 0, or -1 (nothing launched) */
int arthip_ingest_batch (const ArtIngestItem *items, int n, long tasks, void *stream);
/* an item's head for this output address: (address - head * sizeof (art_s)) % 16 == 0 when the address is sample-aligned — pcm_host.c */
int artamd_ingest_head (const void *d_output);

/* ---- lag_products.hip: lagged inner products of whole rows (artamdLagProductsBatchDevice) ----
 * A task is a tile of ART_LAG_TILE consecutive frames of one row; a row's sums are its tiles' partials added in ascending order. */
#define ART_LAG_MAX 8                    /* ARTAMD_LAG_PRODUCTS_MAX: lags 0 .. 7 */
#define ART_LAG_TILE 4096
typedef struct {
    const art_s *u, *v;
    double *sums;                        /* `lags` values */
    long task0;                          /* first task of this row in the call's flattened task space */
    int frames, first, lags, pad;        /* frames > 0; first >= 0, lags >= 1, first + lags <= ART_LAG_MAX */
} ArtLagRow;
/* the checked arguments of artamdLagProductsBatchDevice (`live` rows with numFrames > 0): builds and uploads the table (per-device
 * scratch of the process, with the partials) and enqueues the two launches on `stream`; the launch count, or -1 */
int arthip_lag_products (const art_s *const *d_u, const art_s *const *d_v, const int *frames, const int *first, const int *lags,
                         double *const *d_sums, int n, int live, void *stream);

#ifdef __cplusplus
}
#endif
#endif
