/* pcm_stub_rt.c — a stand-in for everything pcm_host.c links against (45 arthip_* functions of the HIP translation units,
 * artamd_batch_distinct and artamd_shard_plan of resampler_host.c), for tests/test_pcm_host_trace.py: every call is one line of
 * text on stdout, with its arguments, so that two versions of pcm_host.c can be compared call for call and table byte for table
 * byte without a GPU.
 *
 * Device memory is fake: addresses from a bump allocator, 256-byte aligned, never dereferenced (the host layer never does).
 * Page-locked host memory is real and is printed as an allocation number.  Read-backs fill zeros.  Uploaded tables are dumped as hex,
 * or, where the driver asks for it (the variants and failures of a case that is dumped), as a hash of their bytes.  The lane and scratch rules are
 * fixed stand-ins chosen to make padding happen; they do not mirror the product.  stub_fail () makes the k-th call of one
 * function fail. */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "art_internal.h"

#define DEV_BASE  ((uintptr_t) 0x100000000000)       /* the bump allocator's addresses, then the driver's buffers, streams ... */
#define FAKE_END  ((uintptr_t) 0x300000000000)       /* ... everything in [DEV_BASE, FAKE_END) is printed as the number it is */

int stub_quiet;                                      /* 1: nothing is printed (the driver's set-up and tear-down) */
int stub_digest;                                     /* 1: an uploaded table is printed as its length and FNV-1a hash, not dumped (the variants of a dumped case) */
int stub_shards;                                     /* what artamd_shard_plan answers: 0, or that many shards on devices 0, 1 .. */
static const char *fail_fn;
static int fail_at, fail_seen, current_device;
static char last_error [128] = "no error";
static uintptr_t bump = DEV_BASE, handles = (uintptr_t) 0x2e0000000000;
static struct { char *p; size_t bytes; } pinned [512];
static int npinned;

void stub_fail (const char *fn, int at) { fail_fn = fn; fail_at = at; fail_seen = 0; }

/* 1: this call is the one that fails */
static int failing (const char *fn)
{
    if (!fail_fn || strcmp (fn, fail_fn) || ++fail_seen != fail_at) return 0;
    snprintf (last_error, sizeof (last_error), "injected failure of %s", fn);
    return 1;
}
#define FAILS failing (__func__)

static void say (const char *fmt, ...)
{
    va_list ap;
    if (stub_quiet) return;
    va_start (ap, fmt);
    vprintf (fmt, ap);
    va_end (ap);
    putchar ('\n');
}

static int fake (const void *p) { return (uintptr_t) p >= DEV_BASE && (uintptr_t) p < FAKE_END; }

/* a pointer as text: a fake address as it is, page-locked memory as its allocation number and offset, other host memory "host" */
static const char *nm (const void *p)
{
    static char text [16][48];
    static int turn;
    char *s = text [turn++ & 15];
    if (!p) return "0";
    if (fake (p)) { snprintf (s, sizeof (text [0]), "%#llx", (unsigned long long)(uintptr_t) p); return s; }
    for (int k = 0; k < npinned; ++k)
        if (pinned [k].p && (const char *) p >= pinned [k].p && (const char *) p < pinned [k].p + pinned [k].bytes) {
            snprintf (s, sizeof (text [0]), "pin%d+%zu", k, (size_t)((const char *) p - pinned [k].p));
            return s;
        }
    return "host";
}

static void *bump_alloc (size_t bytes)
{
    void *p = (void *) bump;
    bump += (bytes + 255) & ~(uintptr_t) 255;
    if (!bytes) bump += 256;
    return p;
}

/* 16 bytes per line behind their offset; a line of zeros only is left out (the offsets and the table's size tell where they are) */
static void hex_dump (const void *data, size_t bytes)
{
    static const unsigned char zeros [16];
    const unsigned char *b = data;
    if (stub_quiet) return;
    for (size_t at = 0; at < bytes; at += 16) {
        const size_t len = bytes - at < 16 ? bytes - at : 16;
        if (!memcmp (b + at, zeros, len)) continue;
        printf ("  %06zx", at);
        for (size_t k = 0; k < len; ++k) printf (" %02x", b [at + k]);
        putchar ('\n');
    }
}

/* ---- the device, memory, streams and events ---- */
int arthip_device_count (void) { say ("device_count"); return FAILS ? 0 : 2; }
int arthip_current_device (void) { say ("current_device -> %d", current_device); return current_device; }
int arthip_set_device (int device) { say ("set_device %d", device); if (FAILS) return -1; current_device = device; return 0; }
const char *arthip_last_error (void) { return last_error; }

void *arthip_malloc (size_t bytes)
{
    void *p = FAILS ? NULL : bump_alloc (bytes);
    say ("malloc %zu -> %s", bytes, nm (p));
    return p;
}
void arthip_free (void *p) { say ("free %s", nm (p)); }
void *arthip_grow (void *dev, size_t *cap, size_t need)
{
    const int fails = FAILS;
    void *p = dev;
    if (fails) { p = NULL; *cap = 0; }
    else if (need > *cap || !dev) { *cap = need + need / 2; p = bump_alloc (*cap); }
    say ("grow %s need %zu -> %s cap %zu", nm (dev), need, nm (p), *cap);
    return p;
}
void *arthip_host_alloc (size_t bytes)
{
    void *p = FAILS || npinned == (int)(sizeof (pinned) / sizeof (pinned [0])) ? NULL : calloc (1, bytes ? bytes : 1);
    if (p) { pinned [npinned].p = p; pinned [npinned].bytes = bytes ? bytes : 1; ++npinned; }
    say ("host_alloc %zu -> %s", bytes, nm (p));
    return p;
}
void arthip_host_free (void *p)
{
    say ("host_free %s", nm (p));
    for (int k = 0; k < npinned; ++k)
        if (p && pinned [k].p == p) { free (p); pinned [k].p = NULL; }
}
void *arthip_stream_create (void)
{
    void *s = FAILS ? NULL : (void *)(handles += 16);
    say ("stream_create -> %s", nm (s));
    return s;
}
void arthip_stream_destroy (void *stream) { say ("stream_destroy %s", nm (stream)); }
void *arthip_order_event_create (void)
{
    void *e = FAILS ? NULL : (void *)(handles += 16);
    say ("order_event_create -> %s", nm (e));
    return e;
}
void arthip_event_destroy (void *ev) { say ("event_destroy %s", nm (ev)); }
int arthip_event_record (void *ev, void *stream) { say ("event_record %s stream %s", nm (ev), nm (stream)); return FAILS ? -1 : 0; }
int arthip_stream_wait_event (void *stream, void *event) { say ("stream_wait_event %s event %s", nm (stream), nm (event)); return FAILS ? -1 : 0; }
int arthip_sync (void *stream) { say ("sync %s", nm (stream)); return FAILS ? -1 : 0; }

/* ---- copies: what lands in host memory is zeros; a small host source is printed ---- */
static void land (void *dst, size_t bytes) { if (dst && !fake (dst)) memset (dst, 0, bytes); }
static void small_source (const void *src, size_t bytes) { if (src && !fake (src) && bytes <= 16) hex_dump (src, bytes); }

int arthip_h2d (void *dst, const void *src, size_t bytes, void *stream)
{
    say ("h2d %s <- %s bytes %zu stream %s", nm (dst), nm (src), bytes, nm (stream));
    small_source (src, bytes);
    return FAILS ? -1 : 0;
}
int arthip_d2h (void *dst, const void *src, size_t bytes, void *stream)
{
    say ("d2h %s <- %s bytes %zu stream %s", nm (dst), nm (src), bytes, nm (stream));
    land (dst, bytes);
    return FAILS ? -1 : 0;
}
int arthip_d2d (void *dst, const void *src, size_t bytes, void *stream)
{
    say ("d2d %s <- %s bytes %zu stream %s", nm (dst), nm (src), bytes, nm (stream));
    return FAILS ? -1 : 0;
}
int arthip_zero (void *dst, size_t bytes, void *stream) { say ("zero %s bytes %zu stream %s", nm (dst), bytes, nm (stream)); return FAILS ? -1 : 0; }
int arthip_copy2d (void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, void *stream)
{
    say ("copy2d %s pitch %zu <- %s pitch %zu width %zu rows %zu stream %s", nm (dst), dpitch, nm (src), spitch, width, rows, nm (stream));
    return FAILS ? -1 : 0;
}
int arthip_copy_by_kernel (void *dst, const void *src, size_t bytes, void *stream)
{
    say ("copy_by_kernel %s <- %s bytes %zu stream %s", nm (dst), nm (src), bytes, nm (stream));
    land (dst, bytes);
    return FAILS ? -1 : 0;
}
int arthip_copy2_by_kernel (void *dst, const void *src, size_t bytes, void *dst2, const void *src2, size_t bytes2, void *stream)
{
    say ("copy2_by_kernel %s <- %s bytes %zu, %s <- %s bytes %zu stream %s", nm (dst), nm (src), bytes, nm (dst2), nm (src2), bytes2, nm (stream));
    land (dst, bytes); land (dst2, bytes2);
    return FAILS ? -1 : 0;
}
int arthip_slice_copy (void *dst, size_t dpitch_words, const void *src, size_t spitch_words, int width_words, size_t rows, void *stream)
{
    say ("slice_copy %s pitch %zu <- %s pitch %zu width %d rows %zu stream %s", nm (dst), dpitch_words, nm (src), spitch_words, width_words, rows, nm (stream));
    return FAILS ? -1 : 0;
}
int arthip_slice_copy_bytes (void *dst, size_t dpitch, const void *src, size_t spitch, int width, size_t rows, void *stream)
{
    say ("slice_copy_bytes %s pitch %zu <- %s pitch %zu width %d rows %zu stream %s", nm (dst), dpitch, nm (src), spitch, width, rows, nm (stream));
    return FAILS ? -1 : 0;
}
int arthip_table_upload (const void *table, size_t bytes, void *d_table, void *stream)
{
    say ("table_upload bytes %zu -> %s stream %s", bytes, nm (d_table), nm (stream));
    if (stub_digest && !getenv ("PCM_TRACE_DUMP")) {       /* (PCM_TRACE_DUMP=1: every table dumped, to find where a variant's hash comes apart) */
        unsigned long long h = 0xcbf29ce484222325ull;
        for (size_t k = 0; k < bytes; ++k) h = (h ^ ((const unsigned char *) table) [k]) * 0x100000001b3ull;
        say ("  fnv1a %016llx", h);
    }
    else hex_dump (table, bytes);
    return FAILS ? -1 : 0;
}
int arthip_copy_rows_launch (const void *d_items, int n, long tasks, void *stream)
{
    say ("copy_rows_launch items %s n %d tasks %ld stream %s", nm (d_items), n, tasks, nm (stream));
    return FAILS ? -1 : 0;
}

/* ---- decimator ---- */
static void say_dec_args (const char *call, const ArtDecArgs *a)
{
    say ("%s C %d bits %d bytes %d dither_type %d dither_on %d shaping_on %d order %d scale %a feedback %s gens %s gens_next %s shapers %s clipped %s",
         call, a->C, a->bits, a->bytes, a->dither_type, a->dither_on, a->shaping_on, a->shaping_order, (double) a->scale,
         nm (a->feedback), nm (a->gens), nm (a->gens_next), nm (a->shapers), nm (a->clipped));
}
/* (as the product: 1 when the time-parallel form left the generator state in gens_next) */
static int dec_result (const ArtDecArgs *a, int frames) { return frames >= 64 && !a->shaping_on; }

int arthip_decimate (const ArtDecArgs *a, const art_s *d_in, int frames, unsigned char *d_out, void *stream)
{
    say_dec_args ("decimate", a);
    say ("  in %s frames %d out %s stream %s", nm (d_in), frames, nm (d_out), nm (stream));
    return FAILS ? -1 : dec_result (a, frames);
}
int arthip_decimate_pitched (const ArtDecArgs *a, const art_s *d_in, long in_pitch, int frames, unsigned char *d_out, long out_pitch, void *stream)
{
    say_dec_args ("decimate_pitched", a);
    say ("  in %s pitch %ld frames %d out %s pitch %ld stream %s", nm (d_in), in_pitch, frames, nm (d_out), out_pitch, nm (stream));
    return FAILS ? -1 : dec_result (a, frames);
}
int arthip_decimate_planar (const ArtDecArgs *a, const art_s *d_in, long in_pitch, int frames, unsigned char *d_out, long out_pitch, void *stream)
{
    say_dec_args ("decimate_planar", a);
    say ("  in %s pitch %ld frames %d out %s pitch %ld stream %s", nm (d_in), in_pitch, frames, nm (d_out), out_pitch, nm (stream));
    return FAILS ? -1 : 0;
}
int arthip_decimate_batch_lanes (int lanes) { say ("decimate_batch_lanes %d", lanes); return lanes < 16 ? 4 : 8; }
int arthip_decimate_batch_launch (const ArtDecClass *cls, const void *d_table, void *stream)
{
    say ("decimate_batch_launch serial %d order %d dither %d tasks %ld pitched %d clips %d count %d lanes %d offset %zu table %s stream %s",
         cls->serial, cls->order, cls->dither, cls->tasks, cls->pitched, cls->clips, cls->slice.count, cls->slice.lanes, cls->slice.offset,
         nm (d_table), nm (stream));
    return FAILS ? -1 : 0;
}

/* ---- biquad ---- */
int arthip_biquad_chain (Biquad *d_sections, int C, int S, art_s *d_buf, int frames, int stride, void *stream)
{
    say ("biquad_chain sections %s C %d S %d buf %s frames %d stride %d stream %s", nm (d_sections), C, S, nm (d_buf), frames, stride, nm (stream));
    return FAILS ? -1 : 0;
}
int arthip_biquad_order2 (Biquad *d_sections, int C, int S, art_s *d_buf, int frames, int stride, void *stream)
{
    say ("biquad_order2 sections %s C %d S %d buf %s frames %d stride %d stream %s", nm (d_sections), C, S, nm (d_buf), frames, stride, nm (stream));
    return FAILS ? -1 : 0;
}
size_t arthip_biquad_spec_scratch (int C, int S, int frames, int L)
{
    const size_t bytes = 32 * ((size_t) C * S * ((frames + L - 1) / L) + 1);
    say ("biquad_spec_scratch C %d S %d frames %d L %d -> %zu", C, S, frames, L, bytes);
    return bytes;
}
int arthip_biquad_spec_arm (int *d_first_bad, int C, void *stream) { say ("biquad_spec_arm %s C %d stream %s", nm (d_first_bad), C, nm (stream)); return FAILS ? -1 : 0; }
int arthip_biquad_spec (Biquad *d_sections, int C, int S, const art_s *d_in, int in_stride, art_s *d_out, int out_stride, int frames,
                        int L, int W, void *d_states, int *d_first_bad, unsigned int *d_repairs, void *stream)
{
    say ("biquad_spec sections %s C %d S %d in %s stride %d out %s stride %d frames %d L %d W %d states %s first_bad %s repairs %s stream %s",
         nm (d_sections), C, S, nm (d_in), in_stride, nm (d_out), out_stride, frames, L, W, nm (d_states), nm (d_first_bad), nm (d_repairs), nm (stream));
    return FAILS ? -1 : 0;
}
int arthip_biquad_spec_planar (Biquad *d_sections, int C, int S, const art_s *d_in, long in_pitch, art_s *d_out, long out_pitch, int frames,
                               int L, int W, void *d_states, int *d_first_bad, unsigned int *d_repairs, void *stream)
{
    say ("biquad_spec_planar sections %s C %d S %d in %s pitch %ld out %s pitch %ld frames %d L %d W %d states %s first_bad %s repairs %s stream %s",
         nm (d_sections), C, S, nm (d_in), in_pitch, nm (d_out), out_pitch, frames, L, W, nm (d_states), nm (d_first_bad), nm (d_repairs), nm (stream));
    return FAILS ? -1 : 0;
}
int arthip_biquad_batch_lanes (int lanes) { say ("biquad_batch_lanes %d", lanes); return lanes < 8 ? 4 : 8; }
static int bq_class_launch (const char *call, int fails, const ArtBqClass *cls, const void *d_table, int reversed, void *stream)
{
    say ("%s S %d count %d lanes %d offset %zu table %s reversed %d stream %s", call, cls->S, cls->slice.count, cls->slice.lanes, cls->slice.offset,
         nm (d_table), reversed, nm (stream));
    return fails ? -1 : 0;
}
static int bq_clip_class_launch (const char *call, int fails, const ArtBqClipClass *cls, const void *d_table, int reversed, void *stream)
{
    say ("%s S %d planar %d count %d channels %d tasks %ld offset %zu table %s reversed %d stream %s", call, cls->S, cls->planar, cls->count, cls->channels,
         cls->tasks, cls->offset, nm (d_table), reversed, nm (stream));
    return fails ? -1 : 0;
}
int arthip_biquad_batch_launch (const ArtBqClass *cls, const void *d_table, void *stream) { return bq_class_launch ("biquad_batch_launch", FAILS, cls, d_table, 0, stream); }
int arthip_biquad_filter_batch_launch (const ArtBqClass *cls, const void *d_table, int reversed, void *stream) { return bq_class_launch ("biquad_filter_batch_launch", FAILS, cls, d_table, reversed, stream); }
int arthip_biquad_clips_launch (const ArtBqClipClass *cls, const void *d_table, void *stream) { return bq_clip_class_launch ("biquad_clips_launch", FAILS, cls, d_table, 0, stream); }
int arthip_biquad_filter_clips_launch (const ArtBqClipClass *cls, const void *d_table, int reversed, void *stream) { return bq_clip_class_launch ("biquad_filter_clips_launch", FAILS, cls, d_table, reversed, stream); }

/* ---- ingest ---- */
int arthip_ingest (const unsigned char *d_in, art_s gain_factor, int bits, int bytes, int stride, art_s *d_out, int n, void *stream)
{
    say ("ingest in %s gain %a bits %d bytes %d stride %d out %s n %d stream %s", nm (d_in), (double) gain_factor, bits, bytes, stride, nm (d_out), n, nm (stream));
    return FAILS ? -1 : 0;
}
int arthip_ingest_batch (const ArtIngestItem *items, int n, long tasks, void *stream)
{
    say ("ingest_batch n %d tasks %ld stream %s", n, tasks, nm (stream));
    for (int i = 0; i < n; ++i)
        say ("  item %d in %s out %s task0 %ld gain %a bits %d bytes %d stride %d count %d head %d", i, nm (items [i].in), nm (items [i].out), items [i].task0,
             (double) items [i].gain_factor, items [i].bits, items [i].bytes, items [i].stride, items [i].count, items [i].head);
    return FAILS ? -1 : 0;
}

/* ---- resampler_host.c's two ---- */
int artamd_batch_distinct (const void *const *items, int n, unsigned long *(*stamp_of) (const void *item), const char *what, const char *noun)
{
    static unsigned long calls;
    const unsigned long stamp = ++calls;
    int rc = 0;
    for (int i = 0; i < n && !rc; ++i) {
        if (!items [i]) { rc = -1; break; }
        unsigned long *seen = stamp_of (items [i]);
        if (*seen == stamp) rc = -1;
        *seen = stamp;
    }
    say ("batch_distinct n %d what '%s' noun '%s' -> %d", n, what, noun, rc);
    return rc;
}
int artamd_shard_plan (int channels, int home, int *devices_out)
{
    const int count = stub_shards > 1 && stub_shards <= channels ? stub_shards : 0;
    for (int s = 0; s < count; ++s) devices_out [s] = s;
    say ("shard_plan channels %d home %d -> %d", channels, home, count);
    return count;
}
