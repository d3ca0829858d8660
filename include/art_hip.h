/* art_hip.h — MI355X extensions to the reference C API (additive; nothing here exists in the
 * reference).  Device-pointer entry points take HIP device pointers, enqueue their work on the
 * context's stream and return without synchronising: the frame counts in the result are computed
 * on the host by replaying the reference's scalar position state machine
 * (reference resampler.c:487-537) in closed form, so they are available immediately.
 *
 * Devices.  An ordinary context lives on the HIP device that is current when it is created and makes
 * that device current around every call it serves (so `torch.cuda.set_device(LOCAL_RANK)` before
 * resampleInit gives one process per GPU).  A context created with
 * RESAMPLE_MULTITHREADED spreads its channels over several devices INSIDE the one context — the
 * reference's one-worker-per-channel fan-out (reference resampler.c:185-186, :442-470) with GPUs
 * for threads: see artamdSetDevices below.
 */
#ifndef ARTAMD_ART_HIP_H
#define ARTAMD_ART_HIP_H

#include "resampler.h"
#include "biquad.h"
#include "decimator.h"
#include <stddef.h>
#include "stretch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime ---- */
int artamdDeviceCount (void);                       /* 0 when no usable gfx950 device / HIP runtime */
/* device memory and transfers for callers of the device-pointer entry points that bring no GPU runtime of their own (a tool in C,
 * or tools/art_gpu.py without torch): thin names over the HIP runtime; the transfers are asynchronous on `hipStream` (NULL: the
 * null stream) and return 0 on success */
void *artamdDeviceAlloc (size_t bytes);
void artamdDeviceFree (void *d_ptr);
int artamdUpload (void *d_dst, const void *h_src, size_t bytes, void *hipStream);
int artamdDownload (void *h_dst, const void *d_src, size_t bytes, void *hipStream);
int artamdDeviceZero (void *d_dst, size_t bytes, void *hipStream);
int artamdStreamSynchronize (void *hipStream);
const char *artamdVersion (void);

/* Devices that RESAMPLE_MULTITHREADED contexts created from now on spread their channels over (contiguous, balanced
 * channel slices, one shard per listed device; a device may be listed more than once).  count <= 0 restores the default:
 * the environment's ARTAMD_DEVICES="0,1,2,..." list, else every visible device.  With a single device the flag has no
 * effect unless ARTAMD_SHARDS=n forces n shards (several per device: how the sharded path is tested on a one-GPU box).
 * Every shard has its own stream, history and filter-bank replica; no sample crosses between shards.  Host-pointer calls
 * de-interleave each shard's channel slice on the way into its HBM; device-pointer calls take buffers on the device the
 * context was created on and move the slices peer-to-peer.  Returns 0, or -1 for a device that does not exist. */
int artamdSetDevices (const int *devices, int count);
int resampleHipGetDevice (Resample *cxt);            /* the context's device (sharded: where device-pointer buffers are expected) */
int resampleHipNumShards (Resample *cxt);            /* 0 for an ordinary context */
int resampleHipShardInfo (Resample *cxt, int shard, int *device, int *firstChannel, int *numChannels);   /* 0, or -1: no such shard */

/* ---- resampler ---- */
/* default: the null stream.  Work already enqueued on the previous stream is drained before the switch (history and
 * scratch buffers are shared between calls); biquadBankSetStream, decimateHipSetStream and stretchHipSetStream do the same. */
void resampleHipSetStream (Resample *cxt, void *hipStream);
void resampleHipSynchronize (Resample *cxt);
/* kernel selection for tests and comparisons: 0 = automatic, 1 = general kernel, 2 = matrix-core path wherever the ratio is
 * rational (the persistent streaming kernel for regular launches, the one-tile-per-workgroup kernel otherwise; falls back to
 * 1 elsewhere), 5 = as 2 but always the one-tile-per-workgroup f32 kernel, 6 = as 2 but never the fixed-point kernel: the f32
 * streaming kernel for regular launches (5 and 6 give the same bits; the fixed-point kernel rounds once per output and
 * differs from them in the last place), 7 = as 2 and the fixed-point kernel wherever it can run (automatically it takes
 * filters of 512 taps and more in calls of about a billion output-sample taps and more, where it is the faster one).
 * ARTAMD_KERNEL=<n> in the environment is the preference every NEW context starts with (programs that cannot make this call:
 * the reference's own art / artest binaries on this library, tests/test_gpu_pcm_default_mode.py). */
void resampleHipSetKernel (Resample *cxt, int which);
/* (6 on a fixed-ratio stream — resampleFixedRatioInit — also makes the output independent of how the input is cut into calls, bit for bit, as the
 * reference's is: every launch runs the one kernel on tiles anchored on the stream's canonical period.  Calls of at least one period of outputs;
 * device-pointer input aligned to a frame (1 - 2 channels) / 16 bytes (4 and more).  resampler.h's header; tests/test_gpu_cut_invariance.py) */
/* THE CUT-INVARIANT STREAM POLICY (round 6).  The reference's fixed-ratio output is bitwise independent of how the input is cut into calls
 * (resampler.c:323-335, 533-535: `artest -e -b256 | -b1000 | -b4096 | -b65536`, one checksum).  In the default mode this library picks a kernel per
 * CALL (general / f32 matrix cores, K split or not / fixed point), each inside the parity bar with its own last bits.  With this policy on, the
 * arithmetic is chosen per STREAM: every launch of a rational-ratio stream — big, small, shorter than one period, planar or interleaved — runs on the
 * f32 matrix-core streaming kernel, un-split, anchored on the stream's canonical period (an output sits in the same tile row, on the same K chunks
 * and flush points whichever call brought it), and the outputs only a flush can make (the stream's last T/2 x ratio) on the general kernel, whose
 * outputs never depend on the cut either: the same bits for ANY cut into calls, host or device buffers.  (Not yet for the flush of a
 * stream whose phases do not fit its filters: its interpolating position accumulates each call's rounding, and the flush is evaluated
 * there — a few samples differ in the last place with the cut; tests/test_gpu_cut_invariance.py.)  A launch that cannot run anchored (a
 * nearest-filter stream with a slot on a half step, a device buffer not aligned to 16 bytes / one frame, a call of several million frames whose
 * position drift exceeds the kernels' tolerance) is given to the general kernel and COUNTED: resampleHipCutInvariantFallbacks () == 0 says the
 * guarantee held for every output so far.  Equivalent: resampleHipSetKernel (cxt, 9), ARTAMD_KERNEL=9.
 * What it costs against the library's own choice (tools/bench_cut_invariant.py, profiles/r6_cut_invariant.txt): nothing is free — small calls lose the
 * general kernel's short launch, mid-sized calls of long filters the K split, big calls the fixed-point kernel — which is why it is a context
 * setting and not the default.  RESAMPLE_STRICT_ORDER (bit-exact reference order) and preference 1 (the general kernel alone) are cut-invariant too.
 * (4-byte samples.  The 8-byte build has no kept rows: there the setting is preference 2 — use RESAMPLE_STRICT_ORDER or preference 1.) */
void resampleHipSetCutInvariant (Resample *cxt, int on);
unsigned int resampleHipCutInvariantFallbacks (Resample *cxt);
/* The streaming matrix kernels keep their filter rows across the calls of a context (built once for the stream's canonical period; every later
 * launch is anchored on that period: DESIGN.md 4.1) — on by default.  Off: every launch builds its rows from its own positions and anchors its
 * tiles on its own first output, as before round 5 (comparisons of kernel forms bit for bit; ARTAMD_ROWS_CACHE=0 does it for a whole process).
 * Either way a sample is within the parity bar; the two differ in the last place of a few per cent of the samples. */
void resampleHipKeepRows (Resample *cxt, int on);
int  resampleHipLastKernel (Resample *cxt);          /* which kernel produced the bulk of the last call */
/* 1 when the context's last call or block ran inside a launch shared by resampleProcessBatchInterleavedDevice,
 * resampleProcessAndFlushBatchInterleavedDevice, resampleProcessScheduleInterleavedDevice or the other schedule entries below, 0 when it ran as a
 * single call (which streams of a service batch) */
int  resampleHipLastGathered (Resample *cxt);
/* the matrix-core path's fixed-point kernel (regular launches, 4-byte samples): 0 = the last call did not use it, 1 = it ran,
 * 2 = it was enqueued and stood down for the f32 kernel's tile loop (an infinity or a NaN among the frames the launch reads: any finite
 * amplitude is held, the block exponents follow the channel's peak).
 * *pairsPerChunk (may be NULL): digit-pair products issued per 32-tap chunk, 5 .. 13 (5 where both upper digit planes of the rows are zero, + 4 for each that is not).  Synchronises. */
int  resampleHipLastFixedPoint (Resample *cxt, double *pairsPerChunk);
/* the form of the fixed-point kernel the last call's last launch was given to: 0 none, 1 fir_i8_stream_kernel (register-staged: 1 and 2
 * channels), 2 fir_i8_dma_kernel (LDS-DMA staging, 32-slot tiles), 3 fir_i8_slab_kernel (64 x 256 tiles, big launches).
 * All three leave the same bits. */
int  resampleHipLastFixedPointKernel (Resample *cxt);
unsigned int resampleHipLastHandedBack (Resample *cxt);   /* outputs the matrix-core kernels evaluated at their own exact position, off their slot's canonical pattern, so far */
/* HIP-event timing of the dominant FIR kernel only (events recorded on the context's stream immediately
 * before and after that kernel's launch; the fix-up and history kernels are outside the bracket).  Enable, run calls, then read: returns accumulated kernel milliseconds and the launch count
 * since timing was (re-)enabled; the read synchronises. */
void resampleHipSetTiming (Resample *cxt, int enable);
double resampleHipReadTiming (Resample *cxt, int *numLaunches);
/* milliseconds the launches covered by the last resampleHipReadTiming spent BEFORE their dominant kernel (table / staging
 * passes of the matrix-core paths — peak pass + digit-plane pass of the fixed-point kernel — and the gaps between them) */
double resampleHipReadPrepTiming (Resample *cxt);

ResampleResult resampleProcessInterleavedDevice (Resample *cxt, const artsample_t *d_input, int numInputFrames,
                                                 artsample_t *d_output, int numOutputFrames, double ratio);
ResampleResult resampleProcessAndFlushInterleavedDevice (Resample *cxt, const artsample_t *d_input, int numInputFrames,
                                                         artsample_t *d_output, int numOutputFrames, double ratio);
/* Many independent streams, one launch: results [i] and the samples in d_outputs [i] are exactly what
 * resampleProcessInterleavedDevice (cxts [i], d_inputs [i], numInputFrames [i], d_outputs [i], numOutputFrames [i], ratios [i])
 * would have produced.  Contexts whose call the general kernel runs (any ratio per context, default or EXTEND mode, an
 * ordinary call, on the stream of cxts [0]) share launches — a service with hundreds of small-block streams is
 * launch-bound one call at a time.  EXTRAPOLATE_ENDPOINTS streams share them too: an ordinary call after the first output is a
 * plain stream's, and the calls that make a first output put their backward LPC fits, all in one launch, in front of the FIR
 * launches.  Matrix-core calls share launches too (4-byte build): a call that the single call would make as ONE un-split launch of the f32
 * streaming kernel on the context's kept rows — a call large enough for the matrix-core path under kernel preference 6, or under 0 / 2 where
 * that kernel is the library's own choice; every anchored call of a context under the cut-invariant policy, a 441-frame tick or a call
 * shorter than one period included — runs with the other such calls of its shape in one grouped launch: the tiles its own launch would
 * have run, on one grid.  (The intent: N streams pay one launch floor instead of N.  Not measured yet — DESIGN.md 4.6.)  Calls share a launch
 * when they agree in interpolation, channels, taps, the period taken at a time (outputs and inputs), the tiles' K length, slot tiles and centre
 * band, the head's length and zero pad, and whether the pass-through pass follows; the count is taken per such class after every call has been
 * decided, and a class of fewer than two calls is made one by one.  resampleHipLastKernel then reads the matrix-core path's value and
 * resampleHipLastGathered 1.
 * All other calls are simply made one by one: strict mode, flushes, a first output after a rewind of the position, contexts on other
 * streams or devices, sharded contexts, timing on — and the matrix-core calls of any other kind: a stream's first matrix launch (it builds
 * the kept rows), calls for the fixed-point or the K-split kernel, launches that are not regular (the one-tile-per-workgroup kernel's), a
 * nearest-filter stream without a low-pass whose launch substitutes its pass-through samples in the kernel's own epilogue (ARTAMD_PASS_FIXUP_MIN,
 * periods of more than 8192 slots) instead of in the pass behind it, channel counts without a compiled width, device input not aligned to
 * 16 bytes / one frame, resampleHipKeepRows (0), the 8-byte build.  A policy context's call that cannot run anchored is the single call,
 * counted as there (resampleHipCutInvariantFallbacks): the policy's guarantee holds through this entry as through the single call.
 * ARTAMD_BATCH_MATRIX=0 (read once) makes every matrix-core call one by one, as before.  A context may appear only once.  Asynchronous
 * like the single call: counts are returned at once, the samples land on the stream.  Returns 0, or -1 if a launch failed (a failed grouped
 * launch is counted in artamdErrorCount and leaves its contexts { 0, 0 }, positions and histories untouched). */
int resampleProcessBatchInterleavedDevice (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const int *numInputFrames,
                                           artsample_t *const *d_outputs, const int *numOutputFrames, const double *ratios,
                                           ResampleResult *results);
/* Many whole clips (or streams that end), one launch per stage: results [i], the samples in d_outputs [i] and the context's state afterwards
 * (position, flags, history, resampleHipLastKernel) are exactly those of resampleProcessAndFlushInterleavedDevice (cxts [i], d_inputs [i],
 * numInputFrames [i], d_outputs [i], numOutputFrames [i], ratios [i]) — including its early return: a context whose input was not all used, or
 * whose output has no room left, is not flushed.  numInputFrames [i] == 0 with a NULL input is a pure flush.
 * First the ordinary calls, as resampleProcessBatchInterleavedDevice makes them (gathered or one by one).  Then the flushes: those of the
 * contexts that may share a launch (on the stream and device of cxts [0], not sharded, not strict order, timing off; the flush proper always
 * runs on the general kernel, so a clip long enough for the matrix-core path is processed there — in a grouped launch where the process
 * phase gathers it, singly otherwise — and flushed with the others) are gathered —
 * the forward tail fits of ALL EXTRAPOLATE_ENDPOINTS contexts one launch, the prefills of the streams whose first output the flush makes a
 * second, the flushes' FIR with their history rolls a third — and the others (also the flush call of a stream that was flushed before) are
 * made as the single call.  Five launches for any number of gathered contexts of one shape (a FIR launch per kernel variant: channel
 * group, interpolation, accumulator, taps class), and no allocation once warm (the tails live in one buffer of cxts [0]).
 * resampleHipLastGathered is 1 for a context whose flush (or, where none was due, whose ordinary call) ran in a shared launch.  A context may appear only once.  Asynchronous like
 * the single call.  Returns 0 (also for n <= 0); -1 with nothing enqueued and nothing counted if a context is NULL or appears twice; -1 if a
 * launch failed (counted in artamdErrorCount): the contexts of the failed launch stand where they stood before it — a failed process launch
 * leaves them { 0, 0 } and no flush is made for anyone, a failed flush launch leaves them the results of their process call. */
int resampleProcessAndFlushBatchInterleavedDevice (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const int *numInputFrames,
                                                   artsample_t *const *d_outputs, const int *numOutputFrames, const double *ratios,
                                                   ResampleResult *results);
/* Many blocks of ONE stream, one launch.  Makes the same calls as this loop, with the same counts and the same samples bit for bit:
 *     in = d_input; out = d_output;
 *     for (k = 0; k < numBlocks; ++k) {
 *         results [k] = (k == numBlocks - 1 && flushLast ? resampleProcessAndFlushInterleavedDevice : resampleProcessInterleavedDevice)
 *                       (cxt, in, numInputFrames [k], out, numOutputFrames [k], ratios [k]);
 *         in += numInputFrames [k] * C;                  (the blocks are contiguous in ONE device input)
 *         out += results [k].output_generated * C;       (the outputs are packed, one block after another)
 *         if (results [k].input_used != numInputFrames [k]) break;      (a cap too small: no later block is made)
 *     }
 * d_output must hold the sum of numOutputFrames [k] frames.  Returns the number of blocks made (0 .. numBlocks; blocks not made get { 0, 0 }),
 * 0 for numBlocks <= 0, and -1 if a numInputFrames [k] is negative (nothing is enqueued) or a launch failed: the blocks of the failed launch get
 * { 0, 0 }, the stream stands exactly where it stood before that launch, blocks made before it keep their results.  Asynchronous like the
 * single call: the counts are known at once, the samples land on the context's stream.
 * Blocks the single call gives to the general kernel are gathered into runs of one launch and one history roll each; every other block (a
 * flush, a block large enough for the matrix-core path, strict order, an EXTRAPOLATE_ENDPOINTS stream's blocks up to and including its
 * first output — its later blocks are gathered —, the cut-invariant policy on a rational ratio, a sharded context) is made as its single
 * call, between the runs, in stream order.  With timing on (resampleHipSetTiming) a run counts as
 * one launch.
 * What a caller needs: the ratios of the next numBlocks blocks, in advance — an ASRC loop that estimates the drift, or a clock-recovery loop
 * on the host that steers by resampleGetPosition, knows them for the blocks it has buffered.  INTEGRATION.md shows such a loop. */
int resampleProcessScheduleInterleavedDevice (Resample *cxt, int numBlocks, const artsample_t *d_input, const int *numInputFrames,
                                              artsample_t *d_output, const int *numOutputFrames, const double *ratios,
                                              int flushLast, ResampleResult *results);
/* ... on channels-first buffers: exactly resampleProcessScheduleInterleavedDevice on transposed copies.  Pitches in samples, as in
 * resampleProcessPlanarDevice below: channel c is at d_input + c * inputPitch and the blocks' inputs follow one another along every plane;
 * block k's outputs start at frame (sum of output_generated of the blocks before it) of every output plane.  A pitch of 0 means that side is
 * interleaved (both 0: the interleaved entry itself); a pitch may exceed the frames used and need not be a multiple of anything — what lies
 * between a plane's last written frame and the next plane is not touched.  Gathered blocks read and write the planes as they come (the
 * general kernel, and the history roll); a block the interleaved schedule makes as its single call is resampleProcessPlanarDevice /
 * resampleProcessAndFlushPlanarDevice at the block's offset into the planes.  Return value and failure contract as above. */
int resampleProcessSchedulePlanarDevice (Resample *cxt, int numBlocks, const artsample_t *d_input, long inputPitch, const int *numInputFrames,
                                         artsample_t *d_output, long outputPitch, const int *numOutputFrames, const double *ratios,
                                         int flushLast, ResampleResult *results);
/* The block schedules of MANY streams, one launch: N drifting streams with K buffered blocks each pay one launch floor instead of N (a schedule
 * per stream) or K (a batch per block index).  For every i, results [i] (numBlocks [i] entries), the samples in d_outputs [i], the context's
 * state afterwards (position, flags, history, resampleHipLastKernel, resampleHipLastGathered, resampleHipCutInvariantFallbacks) and
 * blocksMade [i] are exactly those of
 *     blocksMade [i] = resampleProcessSchedulePlanarDevice (cxts [i], numBlocks [i], d_inputs [i], inputPitches [i], numInputFrames [i],
 *                                                           d_outputs [i], outputPitches [i], numOutputFrames [i], ratios [i], flushLast [i], results [i]);
 * (the interleaved entry: every pitch 0).  A NULL pitch array: every item interleaved on that side; flushLast may be NULL: none;
 * numBlocks [i] <= 0 makes nothing (blocksMade [i] = 0); a cap too small ends that stream's schedule only.  A context may appear only once.
 * A context shares launches if it is on the stream and device of cxts [0], not sharded, not in strict order and has timing off; of its blocks
 * those the single schedule would gather into runs.  The call goes in rounds: every live stream contributes its next run of gatherable blocks,
 * the round's runs go out together — one launch per kernel variant (channel group, interpolation, accumulator, taps class), every run cut
 * into the tiles of its own launch, the history rolls riding along, one table upload (the table lives with cxts [0]: no allocation once warm)
 * — then every stream whose next block is not gatherable makes it as its single call, and so on.  When every block of every stream is
 * gatherable the whole call is one launch per kernel variant.  A context that shares no launch is its own single schedule call.
 * Returns the number of launches enqueued, a single call or single schedule made on the side counting as one; 0 for n <= 0 or nothing to do;
 * -1 with nothing enqueued and nothing counted if a context is NULL or appears twice or a numInputFrames [i][k] is negative; -1 if a launch
 * failed (counted once in artamdErrorCount): every stream of the failed shared launch stands exactly where it stood before its run of that
 * launch, that run's results are { 0, 0 }, blocksMade [i] counts the blocks made before it, no later block of any stream is made, and blocks
 * made before the failure keep their results.  Asynchronous like the single call. */
int resampleProcessScheduleBatchInterleavedDevice (Resample *const *cxts, int n, const int *numBlocks,
        const artsample_t *const *d_inputs, const int *const *numInputFrames,
        artsample_t *const *d_outputs, const int *const *numOutputFrames, const double *const *ratios,
        const int *flushLast, ResampleResult *const *results, int *blocksMade);
int resampleProcessScheduleBatchPlanarDevice (Resample *const *cxts, int n, const int *numBlocks,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *const *numInputFrames,
        artsample_t *const *d_outputs, const long *outputPitches, const int *const *numOutputFrames,
        const double *const *ratios, const int *flushLast, ResampleResult *const *results, int *blocksMade);
/* planar device buffers: channel c at d_input + c*inputPitch (in samples), likewise output; a pitch of 0 on either side means that side
 * is interleaved.  Big calls are transposed through the context's interleaved staging on the device (the matrix-core kernels read
 * interleaved frames): the same samples as the interleaved entry point's, bit for bit */
ResampleResult resampleProcessPlanarDevice (Resample *cxt, const artsample_t *d_input, long inputPitch, int numInputFrames,
                                            artsample_t *d_output, long outputPitch, int numOutputFrames, double ratio);
/* ... and a whole clip: resampleProcessPlanarDevice, then — unless the input was not all used or the output has no room left, as in
 * resampleProcessAndFlushInterleavedDevice — the flush, which writes behind the process call's frames in every plane (at frame
 * output_generated of the planes; behind the interleaved frames where outputPitch is 0).  The same counts and samples as the interleaved
 * entry point's, bit for bit */
ResampleResult resampleProcessAndFlushPlanarDevice (Resample *cxt, const artsample_t *d_input, long inputPitch, int numInputFrames,
                                                    artsample_t *d_output, long outputPitch, int numOutputFrames, double ratio);
/* Many streams, channels-first buffers (a torch waveform is [C, T], a batch of clips [B, C, Tmax] plus lengths).  The two interleaved batch
 * entries above with a pitch per buffer, in samples, as in resampleProcessPlanarDevice: channel c of item i is at
 * d_inputs [i] + c * inputPitches [i], likewise the output; a pitch of 0 means that side of that item is interleaved, a NULL pitch array that
 * every item's is (both NULL: the interleaved entry itself).  A pitch may exceed the frame count (rows of a padded tensor: what lies between
 * the frames written and the pitch is not touched) and need not be a multiple of 4 samples.  A one-channel context is the same call in either layout.
 * results [i], the samples and the context's state afterwards (position, flags, history), resampleHipLastKernel and
 * resampleHipCutInvariantFallbacks are exactly those of the loop of resampleProcessPlanarDevice (resampleProcessAndFlushPlanarDevice) calls
 * — and so, that call being bit-identical to the interleaved one, those of the interleaved batch entry on transposed copies.
 * Every context decides as its single planar call does.  A call that stays planar (below frames x stream channels x taps = 2e8, no
 * cut-invariant policy) is gathered on the batched general kernel, which reads and writes the planes as they come, its history roll and the
 * EXTRAPOLATE_ENDPOINTS fits likewise.  A call the single call would stage is the interleaved call on the context's own staging, gathered or made
 * singly as the interleaved batch entry would (a grouped matrix-core launch from a stream's second such call on); the inputs of ALL staged calls
 * are transposed by one launch (transpose_group_kernel) in front of the FIR launches, their outputs by one launch behind them: two launches for
 * any number of contexts where the loop of single calls makes two per call.  The flushes always run on the general kernel and write their
 * planes directly.  Contexts that are made one by one (sharded, another stream or device, strict order, timing on) are the single planar call,
 * which stages for itself.  Return values, the failure contract, "a context may appear only once" and asynchronous operation as in the
 * interleaved entries. */
int resampleProcessBatchPlanarDevice (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                      const int *numInputFrames, artsample_t *const *d_outputs, const long *outputPitches,
                                      const int *numOutputFrames, const double *ratios, ResampleResult *results);
int resampleProcessAndFlushBatchPlanarDevice (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                              const int *numInputFrames, artsample_t *const *d_outputs, const long *outputPitches,
                                              const int *numOutputFrames, const double *ratios, ResampleResult *results);
/* Whole clips from a fresh start: exactly resampleReset (cxts [i]) for every i when fromStart != 0, then
 * resampleProcessAndFlushBatchPlanarDevice on the same arguments — the same results, samples and observable context state.  With
 * fromStart == 0 it is that entry.
 * The host part of the reset is resampleReset's own (position, input index, the floor and linear origins, the EXTRAPOLATE_PREFILL
 * history, re-arming a flushed context; the kept filter rows stay).  The device part, for the contexts that share cxts [0]'s stream and
 * device and are not sharded, is ONE launch in front of the batch's: a grouped zeroing kernel (zero_runs_group_kernel) over a table of
 * (pointer, length) runs that rides in the lead context's batch table clears both history buffers of every such context — so it is right
 * for either value of the context's current-buffer index — instead of two memsets per context; once warm it allocates nothing.  Sharded
 * contexts and contexts on another stream or device get their own resampleReset.
 * Refusals and failure as in the batch entry; a refusal (-1: a NULL context or one listed twice) happens before any context is reset.  The
 * reset is made before the batch entry's launches: after one of THOSE failed the contexts stand as after resampleReset.  If the zeroing launch
 * itself cannot be made, the call returns -1 with no context reset and nothing enqueued (counted in artamdErrorCount). */
int resampleProcessAndFlushClipsPlanarDevice (Resample *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                              const int *numInputFrames, artsample_t *const *d_outputs, const long *outputPitches,
                                              const int *numOutputFrames, const double *ratios, int fromStart, ResampleResult *results);
/* The gradient of whole clips: the adjoint (transpose) of what the clips entry above computes.  Per channel, let A_i be the linear map
 * x [numInputFrames [i]] -> y [M_i] that resampleProcessAndFlushClipsPlanarDevice (..., fromStart = 1, ...) applies, with enough room, to a
 * context of the taps, filters, low-pass, flags and fixed ratio of cxts [i] at ratios [i]: the context as resampleReset leaves it, the process
 * call, then the flush; M_i is their total output.  Frames 0 .. numInputFrames [i] - 1 of every plane of d_gradInputs [i] are SET to
 * A_i^T gy_i, where gy_i is the first numOutputFrames [i] frames of d_gradOutputs [i]; the output frames from numOutputFrames [i] up to M_i
 * count as zero gradient (a forward call whose cap cut it short).  Nothing else is written.
 * Pitches as in the sibling entries: in samples, 0 for an interleaved side of an item, a NULL array for "every item is", any pitch and base
 * alignment the sample type allows, a one-channel context the same call in either layout.
 * Every output's position — window start ip - T/2 + 1, filter row fi, frac — is the one the forward kernels' own locate () (fir_common.hip.h)
 * gives it from the planner's segments: two artamdPlanCall replays from a fresh position (the process call, then the flush's call of silence),
 * no context touched.  The weight of output n on input j, k = j - (ip (n) - T/2 + 1):
 *   interpolating     w = (artsample_t)((double) h [fi][k] * (1.0 - frac) + (double) h [fi+1][k] * frac)
 *   nearest filter    w = h [fi][k]; without a low-pass and with fi % F == 0 the reference's pass-through: 1 on the sample it copies, 0 elsewhere
 * and gx [j] = sum over n, ascending, of w * gy [n], one fused multiply-add per term in artsample_t (fir_adjoint.hip is compiled with
 * -ffp-contract=off: nothing else is fused).  (The kernel takes the outputs in groups of four without a branch: between a frame's own terms it
 * may add w * gy [n] with w = 0 for an output of the group whose window does not hold the frame, which leaves a sum of finite terms bit for
 * bit as it was; a non-finite gy [n] may so reach frames next to its window, as it would in a dense product.)  There is ONE arithmetic: the mode flags that only choose the forward's (RESAMPLE_STRICT_ORDER,
 * EXTEND_CONVOLUTION_MATH, the kernel preference, the cut-invariant policy) change nothing here, and gx [j] is the same bit for bit whatever
 * the batch, the item's place in it, the layout, the pitch or the tile of input frames it falls into.  The kernel gathers — a workgroup owns a
 * tile of consecutive input frames and walks the contiguous range of outputs whose windows touch it — so there are no atomics.
 * The contexts are only READ (bank pointer and parameters): no position, history, flag, kept row or resampleHipLast* report changes, and a
 * context may appear any number of times (one context can serve a whole batch).
 * Asynchronous on the stream of cxts [0]; one launch per kernel variant present (channel-group width 1, 2, 4, 8 x interpolating or not),
 * whatever n; the table rides in the lead context's batch table: no allocation once warm.
 * Returns the number of launches enqueued; 0 for n <= 0 and for a list whose every item has numInputFrames [i] == 0 (such an item writes
 * nothing).  -1 with nothing enqueued and nothing counted for a NULL context, a NULL buffer of an item with numInputFrames [i] > 0, a negative
 * count, numOutputFrames [i] > M_i, a context with EXTRAPOLATE_ENDPOINTS (its end-point fits are not linear), a sharded context, a context
 * on another device or stream than cxts [0].  -1 if a launch failed (counted in artamdErrorCount): the gradient buffers are then unspecified.
 * Gradient inputs must not overlap gradient outputs (not checked). */
int resampleAdjointClipsPlanarDevice (Resample *const *cxts, int n,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, const int *numOutputFrames,
        artsample_t *const *d_gradInputs, const long *gradInputPitches, const int *numInputFrames,
        const double *ratios);
/* Whole clips at a rate that changes inside the clip, from a fresh start: exactly resampleReset (cxts [i]) for every i when fromStart != 0,
 * then resampleProcessScheduleBatchPlanarDevice on the same arguments — the same results, samples, blocksMade and observable context state.
 * With fromStart == 0 it is that entry.  The reset is resampleProcessAndFlushClipsPlanarDevice's: the host part resampleReset's own, the
 * device part ONE grouped zeroing launch (zero_runs_group_kernel) over both history buffers of every context that shares cxts [0]'s stream
 * and device and is not sharded, its table in the lead context's batch table — instead of two memsets and a host trip per clip; sharded
 * contexts and contexts on another stream or device get their own resampleReset.
 * Refusals as in the schedule batch entry (-1 with nothing enqueued and nothing counted: a NULL context, one listed twice, a negative
 * numInputFrames [i][k]), before any context is reset.  If the zeroing launch cannot be made the call returns -1 with no context reset and
 * nothing enqueued (counted once in artamdErrorCount).  After a failure of one of the schedule's own launches the contexts it did not reach
 * stand as after resampleReset.  Returns the number of launches enqueued, the zeroing launch counting as one. */
int resampleProcessScheduleClipsPlanarDevice (Resample *const *cxts, int n, const int *numBlocks,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *const *numInputFrames,
        artsample_t *const *d_outputs, const long *outputPitches, const int *const *numOutputFrames,
        const double *const *ratios, const int *flushLast, int fromStart,
        ResampleResult *const *results, int *blocksMade);
/* The gradient of such clips with respect to their samples: the adjoint of what the entry above computes for item i, per channel, with
 * fromStart = 1, flushLast [i] = 1 and room to spare on a context of cxts [i]'s taps, filters, low-pass and flags — numBlocks [i] process
 * calls of numInputFrames [i][k] frames at ratios [i][k], then the flush (at the last block's ratio).  With N_i the sum of the blocks'
 * frames and M_i the total output, frames 0 .. N_i - 1 of every plane of d_gradInputs [i] are SET to A_i^T gy_i, gy_i the first
 * numOutputFrames [i] frames of d_gradOutputs [i] (output frames past that count as zero gradient); nothing else is written.  Pitches as
 * in resampleAdjointClipsPlanarDevice.  For RESAMPLE_FIXED_RATIO contexts `ratios` is ignored (ratios [i] may be NULL), as the forward
 * ignores it.  The ratios get no gradient here: resampleRateGradientScheduleClipsPlanarDevice, below, is theirs.
 * The clip is K + 1 phases, each linear in the samples: K + 1 artamdPlanCall replays on one fresh position (every process call with all
 * the room an int counts, the last the flush's call of silence), each with its own ratio, segments, output count and floor.  Phase k sees
 * input frame j at linear index H + j - s_k (s_k: the frames of the blocks before it; the flush: N_i) and reads nothing below
 * max (0, its floor).  The weight of output n on input j is resampleAdjointClipsPlanarDevice's in all three cases (interpolating, nearest
 * filter, pass-through), every output placed by locate () from its own block's segments and ratio, and gx [j] is the sum over the clip's
 * outputs in ascending order — block by block, then the flush — one fused multiply-add per term in artsample_t (zero weights between a
 * frame's own terms as there).  gx [j] is the same bit for bit whatever the batch, the item's place, the layout, the pitch or the tile;
 * numBlocks [i] = 1 gives resampleAdjointClipsPlanarDevice's bits.  The kernel (fir_adjoint_blocks_kernel) gathers: a workgroup owns a
 * tile of input frames, finds the contiguous range of phases that can touch it by bisection, takes them in groups of 32 (two lanes per
 * phase bisect its output range) and walks each phase as the two-phase kernel does; no atomics.
 * The contexts are only READ, and a context may be listed any number of times.  Asynchronous on the stream of cxts [0]; the items, phases
 * and segments ride in the lead context's batch table in one upload: no allocation on the device once warm.
 * Returns the number of launches enqueued, one per kernel variant present (channel-group width x interpolating or not); 0 for n <= 0 or
 * when every item has N_i == 0 or numBlocks [i] <= 0 (such an item writes nothing).  -1 with nothing enqueued and nothing counted for a
 * NULL context, a NULL buffer of an item with N_i > 0, a NULL block array of an item with numBlocks [i] > 0 (numInputFrames [i]; ratios [i]
 * unless the context is RESAMPLE_FIXED_RATIO — stricter than N_i > 0: an empty clip's M_i depends on its ratio too), a negative count, a ratio that is not > 0, N_i or the clip's
 * output count not fitting an int, numOutputFrames [i] > M_i, a context with EXTRAPOLATE_ENDPOINTS, a sharded context, a context on
 * another device or stream than cxts [0].  -1 if a launch failed (counted once in artamdErrorCount): the gradient buffers are then
 * unspecified.  Gradient inputs must not overlap gradient outputs (not checked). */
int resampleAdjointScheduleClipsPlanarDevice (Resample *const *cxts, int n, const int *numBlocks,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, const int *numOutputFrames,
        artsample_t *const *d_gradInputs, const long *gradInputPitches,
        const int *const *numInputFrames, const double *const *ratios);
/* The gradient of the same clips with respect to their blocks' RATIOS, on contexts with SUBSAMPLE_INTERPOLATE: the clip of item i as in the
 * entry above (a fresh context of cxts [i]'s parameters, the blocks in turn, then the flush at the last block's ratio), x_i the first N_i
 * frames of every plane of d_inputs [i], gy_i the first numOutputFrames [i] frames of d_gradOutputs [i] (output frames past that count as
 * zero gradient and are not read; frames of x_i past N_i are not read).  The numBlocks [i] doubles of d_gradRatios [i] (device memory) are
 * SET to dL/d ratios [i][k] for L = sum gy_i y_i; nothing else is written.  An item with numBlocks [i] <= 0 writes nothing; an empty clip
 * (one block of no frames) gets a zero.  Pitches as in resampleAdjointClipsPlanarDevice.
 * The clip is the K + 1 phases of the entry above; write rho_k for phase k's ratio (rho_k = r_k for k < K, rho_K = r_{K-1}: the flush) and
 * n_k for its output count.  Output n of phase k sits at p = o_k + n / rho_k (n ? n / ratio : 0, as locate () evaluates it), with
 * o_{k+1} = o_k + n_k / rho_k.  It is the lerp of the dot products with bank rows fi and fi + 1, fi = floor (frac (p) F), so it is
 * piecewise linear in p with the slope D = F sum_t (bank [fi + 1][t] - bank [fi][t]) x [ip + t].  THE KINK: on an exact filter boundary
 * (frac F an integer) the derivative is the slope of the cell the forward used — the one locate ()'s floor picks, the upper — and no
 * average is taken.  The output counts n_k, piecewise constant in the ratios, are held fixed.  Then, over the channels and the phase's
 * outputs, S0_k = sum gy D and S1_k = sum n gy D give
 *     dL/d rho_k = -(S1_k + n_k sum_{m > k} S0_m) / rho_k^2,   dL/d r_k = dL/d rho_k (k < K - 1),   dL/d r_{K-1} = dL/d rho_{K-1} + dL/d rho_K.
 * THE TERM ORDER, in fp64 in both builds: per output and channel D = F * (one chain of fused multiply-adds of
 * ((double) bank [fi + 1][t] - (double) bank [fi][t]) and (double) x, t ascending over the taps the phase may read — a tap before the
 * clip, at or past the phase's end or below its floor is left out, not multiplied by zero, so a non-finite neighbour stays out);
 * v = (double) gy * D; the output's pair is (sum_ch v, n * sum_ch v), the channels in order.  The pairs of a tile of 256 consecutive
 * outputs of a phase are added by a butterfly over each wave of 64 and the four waves in order; a phase's tiles in ascending order; the
 * S0 of the phases behind phase k one by one from the flush down; then 0 - (S1_k + n_k * behind) / (rho_k * rho_k), and for the last
 * block dL/d rho_{K-1} + dL/d rho_K in that order.  No atomics: the result is the same bit for bit whatever the batch, the item's place
 * in it, the layout, the pitch or the stream.
 * Two launches (fir_rate_grad.hip: the tiles' partial sums in one flattened task space over the call, then one wave per clip); a phase
 * without outputs has no tile, and a call none of whose phases has an output is the second launch alone.
 * The contexts are only READ, and a context may be listed any number of times.  Asynchronous on the stream of cxts [0]; the items, phases
 * and segments ride in the lead context's batch table in one upload and the tiles' partial sums lie behind them there: no allocation on
 * the device once warm.
 * Returns the number of launches enqueued; 0 for n <= 0 or when every item has numBlocks [i] <= 0.  -1 with nothing enqueued and nothing
 * counted for everything the entry above refuses (d_inputs in the place of its d_gradInputs), a NULL d_gradRatios [i] of an item with
 * blocks, a context without SUBSAMPLE_INTERPOLATE (the nearest filter does not move with the ratio: the gradient would be zero almost
 * everywhere) and a RESAMPLE_FIXED_RATIO context (it ignores the ratios).  -1 if a launch failed (counted once in artamdErrorCount): the
 * gradient buffers are then unspecified. */
int resampleRateGradientScheduleClipsPlanarDevice (Resample *const *cxts, int n, const int *numBlocks,
        const artsample_t *const *d_inputs, const long *inputPitches,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, const int *numOutputFrames,
        const int *const *numInputFrames, const double *const *ratios,
        double *const *d_gradRatios);
/* Whole clips at a POSITION CURVE that lies in device memory — the 1-D, windowed-sinc counterpart of grid_sample: output m of item i is
 * the context's own interpolator evaluated at d_positions [i][m], a double in input frames.  No planner, no context state, no history:
 * cxts [i] supplies T = numTaps, half = T / 2, F = numFilters, its bank and its flags, and is only READ (a context may be listed any
 * number of times; a RESAMPLE_FIXED_RATIO context is taken, only its bank is used).  The output count is the curve's length.
 * For a position p and the N = numInputFrames [i] frames of channel c: whole = floor (p), fr = (p - whole) * F (neither fused); on a
 * SUBSAMPLE_INTERPOLATE context fi = floor (fr), frac = fr - fi, else fi = floor (fr + 0.5), frac = 0; tap t in [0, T) reads input frame
 * whole - half + 1 + t.  This is the position arithmetic of resampleProcess with the offset p: p = 0 is a fresh context's position after
 * resampleAdvancePosition (taps / 2), output m centred on input frame p [m]; p [m] = m / ratio resamples aligned, p [m] = m / ratio - taps / 2
 * is what the clips entries make.  Frames below 0 or at and past N are silence, and their taps are LEFT OUT, not multiplied by zero: a NaN
 * past the clip or in row padding is never read.  A position that is not finite, or with p < -(half + 1) or p >= N + half (compared on
 * the double, before any conversion to int), yields exactly 0, reads nothing and has no term in either gradient.  (Where p - whole rounds
 * up to 1 — a tiny negative p — fi = F is taken as fi = F - 1, frac = 1: the same value, rows inside the bank.)
 *   forward   y [c, m] = (artsample_t)(s0 * (1 - frac) + s1 * frac), s0 and s1 the fp64 dot products with bank rows fi and fi + 1 (one
 *             chain of fused multiply-adds each, t ascending); a nearest-filter context uses s0 alone, and its pass-through case (no
 *             INCLUDE_LOWPASS, fi a multiple of F) is a copy of frame whole + fi / F.
 *   adjoint   gx = A^T gy for the weights A [m, j] = (artsample_t)(h0 * (1 - frac) + h1 * frac) of resampleAdjointClipsPlanarDevice: frames
 *             0 .. N - 1 of every plane of d_gradInputs [i] are SET, the terms added in ascending m, one fused multiply-add each, in
 *             artsample_t.  PRECONDITION: the item's positions do not decrease in m (positions without a window may lie anywhere a
 *             non-decreasing curve of doubles allows; a NaN counts as +infinity).  The outputs whose windows hold frame j are then one
 *             range, found by bisection on the position array itself.  On a curve that decreases somewhere the result is unspecified;
 *             every read and write still stays inside the item's buffers.  (Sort the curve, and gy with it: A^T does not care about the
 *             outputs' order.)
 *   position gradient   the numOutputFrames [i] doubles of d_gradPositions [i] are SET to gp [m] = sum_c gy [c, m] D [c, m] in fp64,
 *             D = F * (one chain of fused multiply-adds of ((double) bank [fi + 1][t] - (double) bank [fi][t]) and (double) x, t
 *             ascending), the channels in order: the slope of the cell floor picks — no average on a filter boundary, and nothing held
 *             fixed.  Contexts with SUBSAMPLE_INTERPOLATE only.
 * Positions are doubles in both sample widths.  Pitches as in resampleProcessBatchPlanarDevice (0, or a NULL pitch list: interleaved).
 * One launch per entry (fir_sample.hip) over one flattened task space — tiles of 256 outputs, or of 256 input frames per channel group —
 * so one long clip and a thousand short ones spread alike; no atomics: every value is the same bit for bit whatever the batch, the
 * item's place in it, the layout, the pitches or the stream.  Asynchronous on the stream of cxts [0]; the items ride in the lead
 * context's batch table.  An item without outputs (the adjoint: or without input frames) is no part of the launch and nothing of it is
 * written: the adjoint zeroes nothing.
 * Returns the number of launches enqueued: 1, or 0 for n <= 0 or when no item is part of the launch.  -1 with nothing enqueued and nothing
 * counted for a NULL context, a context with EXTRAPOLATE_ENDPOINTS, a sharded context, a context on another device or stream than
 * cxts [0], a negative count, numInputFrames [i] > INT_MAX - 2 T, a NULL buffer of an item that is part of the launch (d_inputs [i] only
 * where it has frames), more tiles than an int counts, and — the position gradient — a context without SUBSAMPLE_INTERPOLATE.  -1 if the
 * launch failed (counted once in artamdErrorCount): the outputs are then unspecified.  Outputs must not overlap inputs (not checked). */
int resampleSampleClipsPlanarDevice (Resample *const *cxts, int n,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames,
        const double *const *d_positions, const int *numOutputFrames,
        artsample_t *const *d_outputs, const long *outputPitches);
int resampleSampleAdjointClipsPlanarDevice (Resample *const *cxts, int n,
        const double *const *d_positions, const int *numOutputFrames,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches,
        artsample_t *const *d_gradInputs, const long *gradInputPitches, const int *numInputFrames);
int resampleSamplePositionGradientClipsPlanarDevice (Resample *const *cxts, int n,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames,
        const double *const *d_positions, const int *numOutputFrames,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches,
        double *const *d_gradPositions);
/* The same clips BAND-LIMITED PER OUTPUT from a ladder of banks — what a mip chain is to a texture sampler: where the curve steps faster
 * than one input frame per output, a bank of a lower cut-off keeps the clip from aliasing there, and only there.  cxts holds n * numRungs
 * contexts: rung k of item i is cxts [i * numRungs + k], numRungs = K in 1 .. 8, rung 0 the widest bank by convention — the entries do not
 * look at cut-offs: level k MEANS rung k.  The rungs of an item agree in channels, taps and filters, and every one has SUBSAMPLE_INTERPOLATE
 * (INCLUDE_LOWPASS may differ: resampleInit clears it on a bank without low-pass).  The contexts are only read.  d_levels [i] holds
 * numOutputFrames [i] doubles beside the positions.  The level l of an output:
 *     !(l > 0) — a NaN, -0.0, a negative: L = 0, lam = 0;   l >= K - 1: L = K - 1, lam = 0;   else L = floor (l), lam = l - L.
 * The position arithmetic, the windows and the no-window rule are the sampling entries' above.  With a_k = s0 * (1 - frac) + s1 * frac of
 * rung k in fp64 (the sampling forward's chains and its lerp before the rounding), w_k = h0 * (1 - frac) + h1 * frac in fp64 and D_k the
 * position gradient's D on rung k:
 *   forward    y = (artsample_t) a_L where lam == 0 — rung L + 1 is not read, and the result is resampleSampleClipsPlanarDevice's on rung
 *              L's context bit for bit — else y = (artsample_t)(a_L * (1.0 - lam) + a_{L+1} * lam), nothing fused beyond the chains.
 *              Without a window: exactly 0, nothing read.
 *   adjoint    the transpose: the weight of (output, tap) is rung L's (artsample_t) w_L where lam == 0, else
 *              (artsample_t)(w_L * (1.0 - lam) + w_{L+1} * lam); order, bisection and PRECONDITION (positions that do not decrease) as
 *              resampleSampleAdjointClipsPlanarDevice.  The levels may be anything.
 *   gradients  gp [m] = sum_c gy * D, D = D_L where lam == 0 (resampleSamplePositionGradientClipsPlanarDevice's bits on rung L), else
 *              D_L * (1.0 - lam) + D_{L+1} * lam.  glevel [m] = sum_c gy [c, m] * (a_{j+1} - a_j), j = min (L, K - 2), for
 *              0 <= l <= K - 1, -0.0 included: the closed ends pass the gradient, as a clamp's do, so a level that starts on a rung can
 *              leave it; exactly 0 for l < 0, l > K - 1, a NaN, K = 1 and an output without a window.  d_gradPositions or d_gradLevels
 *              may be NULL — not wanted; the value chains run only where d_gradLevels is given.
 * One launch per entry (fir_sample.hip), the sampling entries' task spaces; an output reads the one or two banks it needs.  The result does
 * not depend on the batch, the layout, the pitches or the stream.  Pitches, n <= 0, the return value (1 or 0 launches) and items without
 * outputs as in the sampling entries.  -1 with nothing enqueued and nothing counted: numRungs outside 1 .. 8, a rung that differs from its
 * item's rung 0 in channels, taps or filters, a rung without SUBSAMPLE_INTERPOLATE, everything the sampling entries refuse (for any rung;
 * d_levels [i] as d_positions [i]), and d_gradPositions and d_gradLevels both NULL. */
int resampleSampleBandClipsPlanarDevice (Resample *const *cxts, int n, int numRungs,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames,
        const double *const *d_positions, const double *const *d_levels, const int *numOutputFrames,
        artsample_t *const *d_outputs, const long *outputPitches);
int resampleSampleBandAdjointClipsPlanarDevice (Resample *const *cxts, int n, int numRungs,
        const double *const *d_positions, const double *const *d_levels, const int *numOutputFrames,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches,
        artsample_t *const *d_gradInputs, const long *gradInputPitches, const int *numInputFrames);
int resampleSampleBandGradientsClipsPlanarDevice (Resample *const *cxts, int n, int numRungs,
        const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames,
        const double *const *d_positions, const double *const *d_levels, const int *numOutputFrames,
        const artsample_t *const *d_gradOutputs, const long *gradOutputPitches,
        double *const *d_gradPositions, double *const *d_gradLevels);

/* ---- host-only building blocks (no GPU needed; used by the CPU test-suite) ---- */
/* (numFilters+1) x numTaps bank exactly as resampleInit builds it (reference resampler.c:149-168, 1090-1133) */
void artamdBuildFilterBank (int numTaps, int numFilters, double lowpassRatio, int flags, artsample_t *bank);

typedef struct {
    unsigned int first_output;      /* outputs [first_output, next.first_output) belong to this segment */
    int lin_base;                   /* ring index + lin_base = index into (history ++ new input) */
    double base_offset;             /* outputOffset valid for this ring epoch */
} ArtamdSegment;

typedef struct {
    int numTaps, numFilters, flags, inputIndex, floorActive;
    double outputOffset, fixedRatio;
} ArtamdPosition;

/* Replay one process call on explicit position state: fills the result, advances *pos and writes up
 * to maxSegments ring-epoch segments.  Returns the number of segments the call needs (may exceed
 * maxSegments; then only the first maxSegments were written).  *linFloor receives the linear index
 * below which history reads as silence (INT_MIN when unrestricted). */
int artamdPlanCall (ArtamdPosition *pos, int numInputFrames, int numOutputFrames, double ratio,
                    ResampleResult *result, ArtamdSegment *segments, int maxSegments, int *linFloor);

/* ---- biquad: device-resident bank of per-channel section chains ---- */
typedef struct artamd_biquad_bank BiquadBank;
/* sections[c*numSections + s] is section s of channel c (state and coefficients are copied) */
BiquadBank *biquadBankCreate (const Biquad *sections, int numChannels, int numSections);
/* the same bank spread over the devices of artamdSetDevices () / ARTAMD_DEVICES (ARTAMD_SHARDS forces the count; at least two
 * channels per device otherwise), contiguous channel slices, one stream per device, the way a RESAMPLE_MULTITHREADED resampler
 * and a DECIMATE_MULTITHREADED decimator spread: same entry points, same bits; an ordinary bank when there is one device */
BiquadBank *biquadBankCreateMulti (const Biquad *sections, int numChannels, int numSections);
int biquadBankShardCount (BiquadBank *bank);         /* 0: an ordinary bank */
void biquadBankSetStream (BiquadBank *bank, void *hipStream);
/* in-place over interleaved device frames [numFrames][numChannels]; asynchronous */
void biquadBankApplyInterleavedDevice (BiquadBank *bank, artsample_t *d_buffer, int numFrames);
void biquadBankRead (BiquadBank *bank, Biquad *sections);      /* synchronises; copies state back */
void biquadBankFree (BiquadBank *bank);
/* Long runs of filters that forget their state within 1,024 frames are computed parallel over TIME, still bit for bit the
 * reference's recurrence: chunks start from a warm-up, every chunk boundary is verified exactly and a mismatch recomputed
 * (pcm_kernels.hip, biquad_spec_kernel).  These report how many chunks had to be recomputed so far (normally 0). */
unsigned int biquadBankRepairs (BiquadBank *bank);   /* synchronises */
unsigned int artamdBiquadRepairs (void);             /* the host-pointer calls (biquad_apply_buffer) of this process */
/* Many independent banks, one launch per section count: the samples in d_buffers [i] and the state biquadBankRead (banks [i])
 * returns afterwards (index included) are exactly those of biquadBankApplyInterleavedDevice (banks [i], d_buffers [i],
 * numFrames [i]), i = 0..n-1.  The cascade is serial per channel, so a stereo stream keeps two lanes of one CU busy; here the
 * channels of many banks share the serial waves, one lane per channel, on the serial form (every form gives the same bits).
 * Banks on the stream and device of banks [0] are gathered; the launches run on that stream.  A sharded bank
 * (biquadBankShardCount > 0), a bank on another stream or device, and a call whose single call would take the time-parallel form
 * and has more than 512 frames (pcm_host.c: BQ_BATCH_SERIAL_MAX, measured) are made as their own single calls, in list order,
 * before the gathered launches.  A bank with numFrames [i] <= 0 is skipped.  In place, interleaved [numFrames][channels]; the
 * buffers of one call must not overlap (not checked).  Asynchronous like the single call.  A gathered call recomputes no chunks,
 * so it adds nothing to biquadBankRepairs.
 * Returns the number of kernel launches enqueued, counting each single call made on the side as one; 0 when n <= 0 or there was
 * nothing to do; -1 with nothing enqueued if a bank appears twice or a pointer in banks is NULL; -1 if a launch failed (counted
 * in artamdErrorCount): the banks of a launch that failed keep their state, and their buffers are left untouched. */
int biquadBankApplyBatchInterleavedDevice (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const int *numFrames);
/* planar device buffers (a torch waveform is [C, T]), in place: channel c at d_buffer + c*pitch (in samples), frame f of a plane at
 * + f; a pitch of 0 means interleaved — the call then IS biquadBankApplyInterleavedDevice — as in decimateProcessPlanarLEDevice.  A
 * pitch may exceed numFrames (rows of a padded tensor: nothing between a plane's last frame and the next plane is read for a result
 * or written) and need not be a multiple of anything; the base needs the sample's own alignment.  A one-channel bank is the same
 * call in either layout.  The samples and the state biquadBankRead returns afterwards (index included) are exactly those of
 * biquadBankApplyInterleavedDevice on the transposed buffer, and a stream may mix the two calls freely.  The call takes the form
 * its interleaved twin would: time-parallel (the planes are first copied aside by one 2-D copy; a lane then fetches and stores its
 * run of a plane 16 bytes at a time, cut at the 16-byte boundaries of the run's own address, so an odd pitch, base or chunk start
 * costs a run a head and a tail of single accesses and nothing else), or serial, on the batch entry's kernel with one lane per
 * plane.  A sharded bank's shards take their run of planes through their slices.  Asynchronous on the bank's stream; numFrames <= 0
 * does nothing. */
void biquadBankApplyPlanarDevice (BiquadBank *bank, artsample_t *d_buffer, long pitch, int numFrames);
/* biquadBankApplyBatchInterleavedDevice with a pitch per item, as in biquadBankApplyPlanarDevice: 0 for an interleaved item, a NULL
 * array for "every item is" (the interleaved entry itself).  Samples and state after the call are exactly those of
 * biquadBankApplyPlanarDevice (banks [i], d_buffers [i], pitches [i], numFrames [i]).  Planar and interleaved items of one section
 * count share the launch of their class (a plane is a lane whose frames are consecutive); sharded banks, banks on another stream or
 * device and calls of more than 512 frames that their single call makes time-parallel are made as their own single planar calls, in
 * list order, before the gathered launches, one launch each in the return value.  Return values, the failure contract, "a bank may
 * appear only once", skipping numFrames [i] <= 0 and asynchronous operation as in the interleaved entry. */
int biquadBankApplyBatchPlanarDevice (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const long *pitches,
                                      const int *numFrames);
/* Whole clips of many banks: biquadBankApplyBatchPlanarDevice whose long time-parallel calls share launches too.  The samples in
 * d_buffers [i], the state biquadBankRead (banks [i]) returns afterwards (index included) and the growth of biquadBankRepairs
 * (banks [i]) are exactly those of biquadBankApplyPlanarDevice (banks [i], d_buffers [i], pitches ? pitches [i] : 0, numFrames [i]),
 * preceded by biquadBankReset (banks [i]) when fromStart != 0 (no copy per bank is made for that: the gathered launches read the
 * bank's first state where it lies, and one launch puts the other banks' sections back).  Pitches as in the batch entry: 0 for an
 * interleaved item, a NULL array for "every item is", a one-channel bank the same call in either layout, any pitch and base.
 * What the batch entry gathers (calls of up to 512 frames, calls shorter than two chunks, filters with no warm-up) goes to its serial
 * launches, one per section count.  The calls it leaves to their single calls because they are time-parallel and long are gathered
 * here: every call keeps the chunk length and warm-up of its single call, and the calls of one section count and one layout share
 * one speculative, one check and one commit launch, behind one copy launch that sets every call's frames aside in scratch memory
 * that lives with banks [0] (no bank grows scratch of its own through this entry).  The calls are taken in list order in rounds
 * that set aside at most 128 MiB each (pcm_host.c: BQ_CLIPS_ROUND_BYTES; a larger call is a round of its own): 1 + 3 launches per
 * class present in a round, at most 25.  Sharded banks and banks on another stream or device than banks [0] are single planar calls,
 * in list order, after their own biquadBankReset when fromStart is set; so is a long time-parallel call that is the only one of the
 * list (one clip: nothing to share).  numFrames [i] <= 0 is skipped; with fromStart the bank is
 * still reset.  In place; the buffers of one call must not overlap (not checked).  Asynchronous on the stream of banks [0].
 * Returns the number of kernel launches enqueued, counting each single call made on the side as one; 0 when n <= 0 or there was
 * nothing to do; -1 with nothing enqueued if a bank appears twice or a pointer in banks is NULL; -1 if memory ran out or a launch
 * failed (counted in artamdErrorCount): nothing is then promised about the buffers and the states of the banks of that round and
 * of the rounds behind it. */
int biquadBankApplyClipsPlanarDevice (BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const long *pitches,
                                      const int *numFrames, int fromStart);
/* Whole clips OUT OF PLACE, forwards or with time reversed: what autograd needs of the stage above (ClipFilter).  Frames
 * 0 .. numFrames [i] - 1 of every channel of d_outs [i] are set to what a bank with banks [i]'s sections, in the state
 * biquadBankCreate left (the first state fromStart reads), makes of d_ins [i]; d_ins [i] is only read.  reversed != 0: time runs
 * backwards — frame numFrames [i] - 1 - m of the output is, bit for bit, frame m of what that fresh bank makes of the sequence
 * u [m] = in [numFrames [i] - 1 - m].  From rest that is the TRANSPOSE of the forward map of the whole clip (a cascade from rest
 * is a product of lower-triangular Toeplitz matrices; they commute, and time reversal on both sides transposes each), so it is the
 * gradient of the forward call.  Pitches as in biquadBankApplyClipsPlanarDevice (0: interleaved; a NULL list: every item is); the
 * two sides' pitches of an item may differ, but both are zero or both are not, unless the bank has one channel.
 * The banks are only READ: no section state, index, mismatch flag or repairs counter of banks [i] is written, so a bank may be
 * listed any number of times (one bank for a whole batch), also while it is in the middle of a stream of its own.  The routes are
 * the clips entry's: more than 512 frames and at least two chunks of a filter that forgets is time-parallel (the chunk cuts of the
 * forward call, made on the reversed sequence when reversed; one speculative, one check and one commit launch per section count and
 * layout, a lone item too), everything else one serial launch per section count.  No copy launch: the kernels read the input where
 * it lies.  The chunk states and the items' mismatch flags live in scratch of banks [0], in rounds of at most 128 MiB of chunk
 * states; chunks that had to be recomputed are added to biquadBankRepairs (banks [0]).  Asynchronous on the stream of banks [0].
 * Returns the number of kernel launches enqueued (0: nothing to do); numFrames [i] <= 0 is skipped.  -1 with nothing enqueued and
 * nothing counted: a NULL bank or buffer of an item with frames, a sharded bank, a bank on another device than banks [0], an item
 * with one side planar and one interleaved (or a pitch that is negative or smaller than its frame count), an item whose input and
 * output ranges overlap.  -1, counted in artamdErrorCount: memory ran out or a launch failed. */
int biquadBankFilterClipsPlanarDevice (BiquadBank *const *banks, int n, const artsample_t *const *d_ins, const long *in_pitches,
                                       artsample_t *const *d_outs, const long *out_pitches, const int *numFrames, int reversed);
/* Puts every section's delay lines and index back to what biquadBankCreate was given (the bank keeps a copy on the device), so that
 * a pool of banks serves clip after clip without biquadBankFree / biquadBankCreate, as decimateHipReset does for decimators.
 * biquadBankRepairs is NOT reset.  Asynchronous on the bank's stream, behind every earlier call; no allocation; sharded banks too. */
void biquadBankReset (BiquadBank *bank);

/* The reference's void entry points (biquad_apply_buffer / _sample, floatIntegersLE) cannot return an error and this library has no
 * CPU path: a failure there (no device, allocation, launch) is printed to stderr, counted, and leaves silence (floatIntegersLE) or the
 * unfiltered samples (biquad) behind.  A tool checks the count before it trusts what it writes; ARTAMD_ABORT_ON_ERROR=1 aborts instead. */
int artamdErrorCount (void);
const char *artamdLastError (void);                  /* NULL while the count is zero */

/* How many periods of an exact rational ratio (outputsPerPeriod = the numerator of the reduced ratio) the matrix-core kernels take at
 * a time: their tiles hold 32 consecutive outputs of one period, so short periods (2x conversions: 2 outputs) or badly fitting ones
 * are taken several at a time — 1 while the padding stays within 15 %.  Informational (the choice is the library's own: the 4-byte
 * build applies the rule with the 64 rows of its fixed-point slab kernel's tiles, which are whole 32-row tiles too — ...Rows (p, 64) —
 * unless ARTAMD_I8_SLAB=0). */
int artamdPeriodMultiple (int outputsPerPeriod);
int artamdPeriodMultipleRows (int outputsPerPeriod, int rows);

/* ---- decimator, device pointers ---- */
void decimateHipSetStream (Decimate *cxt, void *hipStream);
/* asynchronous; clipped-sample count accumulates on the device, read with decimateHipClipped() */
void decimateProcessInterleavedLEDevice (Decimate *cxt, const artsample_t *d_input, int numInputFrames, unsigned char *d_output);
long decimateHipClipped (Decimate *cxt);             /* synchronises; total clipped since init */
/* shards of a DECIMATE_MULTITHREADED context (decimator.h: the reference's one-worker-per-channel fan-out, decimator.c:92-93,
 * 119-136, with devices for threads — ordinary contexts with contiguous channel slices on the devices of artamdSetDevices ());
 * 0: an ordinary context */
int decimateHipShardCount (Decimate *cxt);
/* Many independent decimator contexts, one launch per kind of work: the output bytes, clip counts and state after the call are
 * exactly those of decimateProcessInterleavedLEDevice (cxts [i], d_inputs [i], numInputFrames [i], d_outputs [i]), i = 0..n-1.
 * The error-feedback recurrence is serial per channel, so one stereo stream keeps two lanes of one CU busy; here the channels of
 * many contexts share the serial waves (one launch per shaper order and dither on / off), and contexts without noise shaping of
 * 64 frames and more are one time-parallel launch (by dither on / off).
 * Contexts on the stream and device of cxts [0] are gathered; the launches run on that stream.  A sharded context
 * (decimateHipShardCount > 0), or one on another stream or device, is made as its own single call, in list order.  A context with
 * numInputFrames [i] <= 0 is skipped.  Asynchronous like the single call (clip counts: decimateHipClipped per context); the host
 * mirrors (feedback, tpdf_generators, noise_shapers) are left as the single device call leaves them.
 * Returns the number of kernel launches enqueued, counting each single call made on the side as one; 0 when n <= 0 or there was
 * nothing to do; -1 with nothing enqueued if a context appears twice or a pointer in cxts is NULL; -1 if a launch failed (counted
 * in artamdErrorCount): the contexts of a launch that failed keep their device state and generator buffers as before the call. */
int decimateProcessBatchInterleavedLEDevice (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const int *numInputFrames,
                                             unsigned char *const *d_outputs);
/* planar device buffers (a torch waveform is [C, T]): channel c of the input at d_input + c*inputPitch (in samples), channel c of the
 * output at d_output + c*outputPitch (in BYTES), frame f of an output plane at f*outputBytes; a pitch of 0 on either side means that
 * side is interleaved, as in resampleProcessPlanarDevice.  A pitch may exceed the plane's length (rows of a padded tensor: nothing
 * between a plane's last byte and the next plane is touched) and need not be a multiple of anything; the input needs the sample's own
 * alignment, the output none.  A one-channel context is the same call in either layout.  The output bytes, the clip count and the
 * context's state afterwards are exactly those of decimateProcessInterleavedLEDevice on the transposed input, transposed back, and a
 * stream may mix the two calls freely.  The call runs on the kernel its interleaved twin would (time-parallel without noise shaping
 * from 64 frames on, the LDS-staged serial forms with it): a plane's run of frames is fetched with 16-byte loads and its bytes are
 * stored with whole aligned stores (16 bytes in the time-parallel form, 4 in the serial forms' helper waves), cut at the boundaries
 * of the run's own address, so an odd pitch or base costs a run a head and a tail of single accesses and nothing else.  A sharded
 * context's shards take their run of planes where they lie.  Asynchronous like the interleaved call. */
void decimateProcessPlanarLEDevice (Decimate *cxt, const artsample_t *d_input, long inputPitch, int numInputFrames,
                                    unsigned char *d_output, long outputPitch);
/* decimateProcessBatchInterleavedLEDevice with a pitch per buffer, as in decimateProcessPlanarLEDevice: the input pitches in samples,
 * the output pitches in bytes, 0 for an interleaved side of an item, a NULL pitch array for "every item's is" (both NULL: the
 * interleaved entry itself).  The output bytes, clip counts and state after the call are exactly those of
 * decimateProcessPlanarLEDevice (cxts [i], d_inputs [i], inputPitches [i], numInputFrames [i], d_outputs [i], outputPitches [i]).
 * Planar and interleaved items share the launches of their class (the class count does not grow); sharded contexts and contexts on
 * another stream or device are made as their own single planar calls, in list order.  Return values, the failure contract, "a
 * context may appear only once", skipping numInputFrames [i] <= 0 and asynchronous operation as in the interleaved entry. */
int decimateProcessBatchPlanarLEDevice (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                        const int *numInputFrames, unsigned char *const *d_outputs, const long *outputPitches);
/* Puts the context back to what decimateInit left — error feedback zero, dither generators re-seeded, shaper histories empty, on
 * the device and in the host mirrors (feedback, tpdf_generators, noise_shapers) — so that a pool of contexts serves clip after clip
 * without decimateFree / decimateInit.  The clip counter is NOT reset (decimateHipClipped: total since init).  Asynchronous on the
 * context's stream, behind every earlier call; no allocation; sharded contexts too. */
void decimateHipReset (Decimate *cxt);
/* Whole clips from a fresh start, in the batch entry's shared launches.  For every item i the call leaves exactly what
 *     if (fromStart) decimateHipReset (cxts [i]);
 *     decimateProcessPlanarLEDevice (cxts [i], d_inputs [i], inputPitches ? inputPitches [i] : 0, numInputFrames [i],
 *                                    d_outputs [i], outputPitches ? outputPitches [i] : 0);
 * leaves: the output bytes, the context's running clip total (decimateHipClipped), the device state, the host mirrors (feedback,
 * tpdf_generators, noise_shapers) and which of the two generator arrays is live.  Pitches as in decimateProcessBatchPlanarLEDevice.
 * An item with numInputFrames [i] <= 0 is skipped; with fromStart its context is still put back.  fromStart == 0 with
 * d_clipCounts == NULL is decimateProcessBatchPlanarLEDevice itself.
 * No operation per context: the gathered launches (the contexts on the stream and device of cxts [0] that are not sharded) read
 * every context's first values from the image decimateInit left, where it lies, and write the live state; no copy, memset or
 * launch is issued per gathered context and nothing in the gathered path synchronises.  (They are kernels of their
 * own — the batch entry's kernel bodies over records of their own; the batch entry's kernels and tables are what they were.)  Zero-frame contexts that
 * are only put back share ONE grouped copy launch, whatever their number.
 * d_clipCounts: NULL, or n entries of device memory on cxts [0]'s device.  Entry i is SET to the number of samples of item i this
 * call clipped (skipped items: 0): the call clears the n entries with one operation on cxts [0]'s stream, and the gathered
 * kernels add what they add to the context's total to the item's entry as well.  Read all of them with one download, in stream
 * order behind the call.
 * Contexts made on the side — sharded contexts and contexts on another stream or device than cxts [0] — get their own
 * decimateHipReset (with fromStart) and their single planar call, in list order; with d_clipCounts their entry is the difference
 * of decimateHipClipped after and before, uploaded on cxts [0]'s stream: this rare path SYNCHRONISES (that context's stream, and
 * cxts [0]'s).
 * Returns the launch count of decimateProcessBatchPlanarLEDevice for the same list, plus one when d_clipCounts is cleared, plus
 * one when fromStart meets zero-frame gathered contexts (their grouped copy): it does not depend on n within a class.  0 for
 * n <= 0; -1 with nothing enqueued, nothing reset and nothing counted if a context is NULL or listed twice; -1 if a launch failed
 * (counted in artamdErrorCount): no separate reset was issued, so the contexts of the failed launch keep the device state, the
 * mirrors and the generator arrays they had before the call. */
int decimateProcessClipsPlanarLEDevice (Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches,
                                        const int *numInputFrames, unsigned char *const *d_outputs, const long *outputPitches,
                                        int fromStart, unsigned long long *d_clipCounts);
void floatIntegersLEDevice (const unsigned char *d_input, double inputGain, int inputBits, int inputBytes, int inputStride,
                            artsample_t *d_output, int numSamples, void *hipStream);
/* Many buffers' integer PCM to samples in ONE launch: item i leaves exactly the bits of floatIntegersLEDevice (d_inputs [i],
 * inputGains [i], inputBits [i], inputBytes [i], inputStrides [i], d_outputs [i], numSamples [i], hipStream), in both builds.  Items
 * the single call ignores (numSamples [i] <= 0, inputBits [i] > 24) are skipped and their outputs not touched.  Inputs may alias
 * each other (one PCM buffer read with two gains); outputs must not overlap (not checked).  Asynchronous on hipStream (NULL: the
 * null stream), on the current device, like the single call; the argument arrays may be reused as soon as the call returns.
 * Returns the number of kernel launches enqueued (1); 0 when n <= 0 or every item is skipped; -1 with nothing enqueued if a live
 * item has a NULL input or output pointer; -1 if the launch failed (counted in artamdErrorCount). */
int floatIntegersBatchLEDevice (const unsigned char *const *d_inputs, const double *inputGains, const int *inputBits,
                                const int *inputBytes, const int *inputStrides, artsample_t *const *d_outputs,
                                const int *numSamples, int n, void *hipStream);

/* ---- end-point extrapolation, device pointers ---- */
/* the most known samples one run may have: the resampler extrapolates from at most numTaps - 1 (LDS holds the run) */
#define ARTAMD_EXTRAPOLATE_MAX_KNOWN 1023
/* LPC extrapolation (the fit EXTRAPOLATE_ENDPOINTS uses), n independent runs in one launch on hipStream.  Run i: counts [i] known
 * samples, oldest first, at d_known [i] + j * strides [i]; backward [i] == 0 writes extras [i] samples that continue past the newest
 * (reference extrapolate_forward), != 0 the extras [i] samples that precede the oldest, nearest first (extrapolate_reverse), to
 * d_out [i] + j * strides [i].  Bit-identical to the reference.  Returns 0, or -1 (nothing enqueued) on a bad argument.
 * Bad: counts [i] < 8 or > ARTAMD_EXTRAPOLATE_MAX_KNOWN, extras [i] < 0, strides [i] < 1, a NULL pointer of a run with extras [i] > 0.
 * n <= 0 does nothing and returns 0; runs with extras [i] == 0 write nothing.  One workgroup per run, on the current device,
 * asynchronous; the argument arrays may be reused as soon as the call returns.  A failed launch returns -1 and is counted in
 * artamdErrorCount.  The known samples of a run must not overlap its own or another run's output (not checked). */
int artamdExtrapolateBatchDevice (const artsample_t *const *d_known, const int *counts, const int *strides, const int *backward,
                                  artsample_t *const *d_out, const int *extras, int n, void *hipStream);

/* ---- lagged inner products of whole rows, device pointers ---- */
/* one more than the largest lag a row may ask for (lags 0 .. 7: a section's a0..a4 and b1..b4 need 0..4 and 1..4) */
#define ARTAMD_LAG_PRODUCTS_MAX 8
/* Lagged inner products of n rows in shared launches: what the coefficient gradients of a biquad cascade are made of (ClipBiquad).
 * Row i, for k = firstLags [i] .. firstLags [i] + numLags [i] - 1:
 *     d_sums [i][k - firstLags [i]] is SET to sum_{t = k}^{numFrames [i] - 1} (double) d_u [i][t] * (double) d_v [i][t - k]
 * Rows are planes with stride 1 (a plane is an item, as in floatIntegersBatchLEDevice), aligned to their sample size; d_u [i] and
 * d_v [i] are only read and may be one row.  A lag k >= numFrames [i] is set to 0; a row with numFrames [i] <= 0 is skipped and its
 * sums are not touched.  Products and sums are fp64 in both builds (the 4-byte build's products are exact) and the output is
 * double in both; no floating-point atomics.
 * Deterministic: a row is cut into tiles of one fixed length, each tile's partial is one fixed tree over the row's frames, and a
 * row's sum is its tiles' partials added in ascending tile order — so the bits of a row's sums do not depend on the other rows of
 * the call, the row's place in the list, the base alignment of d_u [i] and d_v [i] (16-byte loads where the address allows, single
 * accesses at the head and the tail) or the stream.
 * Work is spread over (row, tile) tasks, so a few long rows fill the chip as many short ones do: one launch for the tiles'
 * partials and one small launch that finishes every row.  The table and the partials live in per-device scratch of the process,
 * grown under a lock (calls of different threads take turns to enqueue; a call on another stream than the last one's waits for it
 * on the device); nothing is allocated once warm.  Asynchronous on hipStream (NULL: the null stream), on the current device, like
 * floatIntegersBatchLEDevice; the argument arrays may be reused as soon as the call returns.
 * Returns the number of kernel launches enqueued (2); 0 when n <= 0 or every row is skipped; -1 with nothing enqueued and nothing
 * counted if a live row has a NULL pointer, firstLags [i] < 0, numLags [i] < 1 or firstLags [i] + numLags [i] >
 * ARTAMD_LAG_PRODUCTS_MAX (or an argument array is NULL); -1 if memory ran out or a launch failed (counted in artamdErrorCount). */
int artamdLagProductsBatchDevice (const artsample_t *const *d_u, const artsample_t *const *d_v, const int *numFrames,
                                  const int *firstLags, const int *numLags, double *const *d_sums, int n, void *hipStream);

/* ---- time stretcher, device pointers (stretch.h) ---- */
void stretchHipSetStream (Stretch *cxt, void *hipStream);
/* as stretchProcess / stretchFlush with `samples` / `output` in device memory; both wait for the call to finish (the frame
 * count is the return value).  d_output must hold stretchGetOutputCapacity() frames. */
int stretchProcessDevice (Stretch *cxt, const artsample_t *d_samples, int num_samples, artsample_t *d_output, double ratio);
int stretchFlushDevice (Stretch *cxt, artsample_t *d_output);
/* The stretcher is one serial state machine per stream, so the GPU earns its keep on MANY streams: these make the call
 * above on n independent contexts in ONE launch, one workgroup per context (results identical to n separate calls; the
 * launch uses the stream of cxts[0]; a context may appear only once).  produced[i] = frames written to d_outputs[i].
 * Return 0, or -1 if the launch failed (nothing is then known about the contexts' state). */
int stretchProcessBatchDevice (Stretch *const *cxts, int n, const artsample_t *const *d_samples, const int *num_samples,
                               artsample_t *const *d_outputs, const double *ratios, int *produced);
int stretchFlushBatchDevice (Stretch *const *cxts, int n, artsample_t *const *d_outputs, int *produced);
/* Whole clips, channels-first or interleaved, in ONE launch and ONE synchronisation for any number of clips: for item i exactly
 * stretchProcessDevice (cxts[i], ..., num_samples[i], ..., ratios[i]) (skipped when num_samples[i] <= 0) followed by
 * stretchFlushDevice calls until one returns 0 (four at the most), made on interleaved copies with the outputs behind one
 * another: the same samples, produced[i] = their total in frames, the same context state afterwards.  So it also finishes a stream that
 * earlier single or batched calls began.  fromStart != 0: the same on a context as stretchInit left it, the accumulated length error
 * (outsamples_error) at zero too — stretchReset does NOT zero that, as the reference's does not; so a pool of contexts serves clip
 * after clip and gives what fresh contexts give, with no reset call in between.  Afterwards the context is flushed: terminal, as in the
 * reference, until stretchReset or another fromStart call.
 * Channel c of item i's input is at d_samples[i] + c * inputPitches[i] samples, of its output at d_outputs[i] + c * outputPitches[i];
 * a pitch of 0: that side of that item is interleaved; a NULL pitch array: every item's is.  One channel is the same call in either
 * layout.  A pitch need not be a multiple of anything, and nothing between a plane's last written frame and the next plane is touched;
 * with two channels a non-zero input pitch must be at least num_samples[i] and a non-zero output pitch at least the capacity below;
 * with one channel a pitch is ignored.
 * The launch runs on the stream of cxts[0]; the call waits for it (the counts come from the device).
 * Returns 0 (also for n <= 0).  Returns -1 with nothing enqueued and no state changed for a NULL context, a context listed twice, an
 * item with a NULL output, or a NULL input and num_samples[i] > 0, a pitch too short (or negative), or outputCaps[i] (frames) below artamdStretchClipCapacity for that
 * context's longest period, flags, num_samples[i] and ratios[i]: the device code does not check bounds.  Returns -1 if the launch
 * failed (counted in artamdErrorCount; nothing is then known about the contexts' state). */
int stretchProcessAndFlushBatchPlanarDevice (Stretch *const *cxts, int n, const artsample_t *const *d_samples, const long *inputPitches,
                                             const int *num_samples, artsample_t *const *d_outputs, const long *outputPitches,
                                             const int *outputCaps, const double *ratios, int fromStart, int *produced);
/* frames a whole clip (the process call plus every flush) can emit at most, for a context made with this longest period (frames, as
 * given to stretchInit) and these flags, from any state it can be in: per stage ceil ((in + ring) * max (1, ceil (2 r) / 2)), r the
 * stage's clipped ratio, ring = longest period * 3 (4 with STRETCH_FAST_FLAG), the two stages of a STRETCH_DUAL_FLAG pair chained.
 * Host arithmetic only: no context, no device.  -1: a longest period out of range, or more frames than an int holds. */
int artamdStretchClipCapacity (int longest_period, int flags, int num_samples, double ratio);

/* ---- the splice log and the gradient of whole stretched clips ---- */
/* What a stage of the stretcher did to a whole clip from a fresh start, as the list of its splices.  Every output value of a stage is a
 * copy of one value of its input stream or a cross-fade of two, so with the period search's choices held fixed the stage is a sparse
 * linear map y = A x with at most two non-zeros per row, and the log IS that map.  Indices count VALUES (frame * channels + channel),
 * as the kernel indexes its rings: with two channels the fade weight of value i differs between the two channels of a frame.
 *   to == ARTAMD_STRETCH_COPY   y [out + i] = x [from + i]                                                  for 0 <= i < count
 *   otherwise (a fade)          y [out + i] = (x [from + i] * (count - i) + x [to + i] * i) / count          (artsample_t, unfused)
 * `from` / `to` are relative to the first value of the stage's input stream; negative indices are the silence stretchInit leaves in
 * front of the mark (at most one longest period) and read as zero.  Segments lie in output order and partition the stage's output:
 * out of each is out + count of the one before, the first is 0, no count is 0; `from` never falls from a segment to the next.  A
 * cascaded pair (STRETCH_DUAL_FLAG) has two logs: stage 2's input stream is stage 1's output stream, in the order it was handed over. */
#define ARTAMD_STRETCH_COPY  (-2147483647 - 1)
typedef struct { int out, count, from, to; } ArtamdStretchSegment;   /* 16 bytes */
/* segments stage `stage` (0, or 1: the second of a STRETCH_DUAL_FLAG pair) of a context made with these periods (frames, as given to
 * stretchInit) and flags can write for a clip of num_samples frames at this ratio, from a fresh start.  A step moves the mark on by at
 * least one shortest period and writes three segments at the most, so a stage that is fed n frames writes at most 3 * (n / shortest)
 * of them in steps; the rest is one segment per time the stage is fed (the pass-through of a ratio of 1) and one per flush.  Stage 0 is
 * fed once, num_samples frames, and flushed four times at the most; stage 1 is fed once per step of stage 0, once by its pass-through
 * and once per flush, in all no more than the bound artamdStretchClipCapacity chains for stage 0's output, and flushed four times.
 * Host arithmetic only.  0 for stage 1 without STRETCH_DUAL_FLAG; -1 where artamdStretchClipCapacity gives -1, for a shortest period
 * below 1, a stage other than 0 or 1, or more than an int holds. */
int artamdStretchLogCapacity (int shortest_period, int longest_period, int flags, int num_samples, double ratio, int stage);
/* stretchProcessAndFlushBatchPlanarDevice (..., fromStart = 1, ...) that also writes the logs: the same kernel body with the records
 * added, so the outputs, produced [] and the state left in the contexts are bit for bit that entry's; still one launch and one
 * synchronisation.  d_logs: 2 n device pointers, item i's stages at [2 i] and [2 i + 1] (the second ignored, and may be NULL, for a
 * single stage); logCaps: 2 n capacities in segments; logCounts: 2 n counts, host memory, filled from the read-back that brings
 * produced [] (0 for the absent second stage).  Only clips from a fresh start are logged: a context that continues an earlier call has
 * no well-defined map of its own.
 * Returns as that entry.  Refuses (-1, nothing enqueued, nothing counted in artamdErrorCount) what that entry refuses, and a NULL d_logs,
 * logCaps or logCounts, a NULL log of a stage the context has, or a logCaps entry below artamdStretchLogCapacity: the device code does
 * not check bounds. */
int stretchProcessAndFlushLoggedBatchPlanarDevice (Stretch *const *cxts, int n, const artsample_t *const *d_samples, const long *inputPitches,
                                                   const int *num_samples, artsample_t *const *d_outputs, const long *outputPitches,
                                                   const int *outputCaps, const double *ratios, int *produced,
                                                   ArtamdStretchSegment *const *d_logs, const int *logCaps, int *logCounts);
/* The gradient of logged clips.  Item i: frames 0 .. n_ins [i] - 1 of every channel of d_gins [i] are SET to A_i^T applied to the first
 * n_outs [i] frames of d_gouts [i], A_i the map of the logs at d_logs [2 i], [2 i + 1] with logCounts [2 i], [2 i + 1] segments (as the
 * logged entry left them; for a pair A_i = A2 A1); nothing else is written.  Pitches as in the forward: in samples, 0 for an interleaved
 * side of an item, a NULL array for "every item is"; one channel is the same call in either layout.
 * The contract, per stage, for input value v (C = channels):
 *   a term of v is (gy [o] * (artsample_t) w) / (artsample_t) count for each fade with v = from + i (w = count - i) or v = to + i (w = i),
 *   o = out + i, 0 <= i < count — two roundings, weights of zero included — and gy [o] itself for a copy;
 *   gx [v] is the sum of v's terms in ascending o, each added with a plain addition (no contraction), from +0;
 *   terms with o >= n_outs [i] * C are dropped; a value no segment reads is exactly 0.
 * So gx [v] does not depend on the batch, the item's place in it, the layouts, the tile or the chunking.  The kernel gathers: a workgroup
 * owns a tile of consecutive input values, and walks the one contiguous range of the log that can touch it — no atomics.
 * For a pair the gradient of the intermediate stream (as many values as stage 1 made: the end of its last segment, read from the log on
 * the device) is scratch of cxts [0], sized by what stage 1 can make of n_ins [i] frames at its largest ratio.
 * The contexts are only READ (channels, stage count, periods, and the stream and scratch of cxts [0]): one context may be listed any
 * number of times.  Asynchronous on the stream of cxts [0].  Launches: one per stage present in the batch — the stage that wrote the
 * output for every item, then the first stage of the pairs — two at the most whatever n; their number is returned; an item with
 * n_ins [i] == 0 writes nothing and launches nothing.  0 for n <= 0.
 * -1 with nothing enqueued and nothing counted for a NULL list (pitch arrays apart), a NULL context, a NULL log of a stage the context
 * has, a negative count, a logCounts entry above artamdStretchLogCapacity for n_ins [i] frames at a ratio of 2 (no log of such a clip is
 * that long), a NULL gradient buffer of an item with n_ins [i] > 0, and with two channels a non-zero pitch below the item's
 * frames on that side.  -1 if a launch failed (counted in artamdErrorCount): the gradient buffers are then unspecified.
 * Gradient inputs must not overlap gradient outputs or the logs (not checked). */
int stretchAdjointClipsPlanarDevice (Stretch *const *cxts, int n, const ArtamdStretchSegment *const *d_logs, const int *logCounts,
                                     const artsample_t *const *d_gouts, const long *goutPitches, const int *n_outs,
                                     artsample_t *const *d_gins, const long *ginPitches, const int *n_ins);

#ifdef __cplusplus
}
#endif
#endif
