// pcm_dec_serial_row.inc — phase B of the pipelined decimator kernels (decimate_pipe_kernel, decimate_batch_pipe_kernel), included in
// place by both: one lane takes the nf frames of its row of the LDS tile `tile` (already times the gain: phase A) through the
// error-feedback recurrence and leaves the rounded code values there.  Eight frames per step, by 16-byte LDS accesses.
// Text and not a function: as a function it moved the batch kernel's resource rows in the 8-byte build (profiles/pcm_shared_parts.txt).
// Reads ORDER, DITHER, tile, dth, tid, pitch, nf; updates fb and sh.
{
    auto one = [&] (art_s smp, art_s dither) -> art_s {
        const art_s scaled = smp;                       // already times `scale` (phase A)
        const art_s code = scaled - fb;
        const art_s dithered = code + dither;
        const art_s qf = round_half_up (dithered);
        if (ORDER) { const art_s err = qf - code; fb = shaper_step<ORDER> (sh, err); }
        return qf;
    };
    typedef art_s vec4 __attribute__ ((ext_vector_type (4)));
    art_s *row = tile + tid * pitch;
    const art_s *my_dither = dth + tid * pitch;
    int f = 0;
    for (; f + 8 <= nf; f += 8) {
        vec4 xa = *reinterpret_cast<const vec4 *> (row + f), xb = *reinterpret_cast<const vec4 *> (row + f + 4), da, db;
        if (DITHER) { da = *reinterpret_cast<const vec4 *> (my_dither + f); db = *reinterpret_cast<const vec4 *> (my_dither + f + 4); }
        else { da = (art_s) 0; db = (art_s) 0; }
#pragma unroll
        for (int u = 0; u < 4; ++u) xa [u] = one (xa [u], da [u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) xb [u] = one (xb [u], db [u]);
        *reinterpret_cast<vec4 *> (row + f) = xa; *reinterpret_cast<vec4 *> (row + f + 4) = xb;
    }
    for (; f < nf; ++f) row [f] = one (row [f], DITHER ? my_dither [f] : (art_s) 0);
}
