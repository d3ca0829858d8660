// fir_i8_tile32.inc — the text the two 32-slot fixed-point kernels (fir_i8_stream_kernel, fir_i8_dma_kernel: fir_matrix_i8.hip) share, each part
// stated ONCE.  Shared as text, like fir_matrix_stream_body.inc, not as functions: the K loop of these kernels sits at 128 of 128 registers, and every
// helper function tried in its place — inlined or not — moved the compiler's register allocation (profiles/i8_shared_parts.txt); as text
// every instantiation keeps its registers, spills and occupancy.  A kernel defines I8_PART and includes the file where the part belongs; what a part expects in scope is said with it.
// Both kernels: CG, PASS, PPW, THREADS; a, g, q, wgs_per_xcd; tid, lane, wave; the LDS arrays As_ and Bs_.
#if I8_PART == 1
// ---- prologue: the roll workgroups, the stand-by, this workgroup's place and its list of tiles

const unsigned int stream_blocks = 8u * (unsigned int) wgs_per_xcd;
if (blockIdx.x >= stream_blocks) {                        // extra workgroups: the history roll (as in fir_mfma_kernel)
    if (a.roll_dst) {
        const int e = (int)(blockIdx.x - stream_blocks) * THREADS + tid;
        if (e < a.H * a.C) matrix_roll (a.roll_dst, a.hist, a.in, a.in_frames, a.H, a.C, a.roll_appended, e);
    }
    return;
}
// Samples the digits cannot hold (flag raised by the staging pass; uniform): the launch is produced in f32 by the streaming
// kernel's own tile loop on this kernel's workgroups and LDS (its 2 x 32 rows and 2 x 128 columns of 36 floats fit the
// digit buffers), from the tables the staging pass has left for it — the bits of fir_mfma_stream_kernel.
if (*q.flag == q.epoch) {
    static_assert (sizeof (As_) >= 2 * 32 * MF_LD * sizeof (float) && sizeof (Bs_) >= 2 * MF_COLS * MF_LD * sizeof (float), "the f32 tiles live in the digit buffers");
    stand_by_tiles<CG, PASS> (a, g, wgs_per_xcd, *reinterpret_cast<float (*) [2] [32 * MF_LD]> (&As_), *reinterpret_cast<float (*) [2] [MF_COLS * MF_LD]> (&Bs_));
    return;
}

const int xcd = blockIdx.x & 7, rank = blockIdx.x >> 3;
const int tiles_per_xcd = q.sg_per_xcd * q.g * q.tiles;
const int nchunks = q.ktot / I8_KC;

// tile `within` of this XCD's list -> (slot tile, first period); false if the tile holds no output of the launch
auto tile_at = [&] (int within, int &st, int &j0) -> bool {
    st = within % q.tiles;
    const int t2 = within / q.tiles, jr = t2 % q.g, sg = xcd * q.sg_per_xcd + t2 / q.g;
    if (sg >= q.super_groups) return false;
    j0 = sg * q.g * PPW + jr;
    return a.n_begin + (unsigned int) j0 * g.P + (unsigned int)(st * 32) < a.n_end;
};
int my_tiles = 0;
{ int st, j0; for (int w = rank; w < tiles_per_xcd; w += wgs_per_xcd) my_tiles += tile_at (w, st, j0) ? 1 : 0; }
if (my_tiles == 0) return;
#elif I8_PART == 2
// ---- staging waves: the stream of this workgroup's tiles and where each tile's operands are staged from.  Expects A_STEP (the rows' bytes per chunk),
// NB staged units per thread with bper [u] = the unit's column, in periods behind the tile's first, and bdel [u] to receive its offset; tile_w0 = the tile
// table, its type choosing how an entry is read (i8_table_entry)

// a column whose period lies d exponent blocks behind the tile's first column stages from that block's own planes: d regions
// further on, where the same 4-frame block sits d * eb_step blocks earlier
const unsigned int x_total = 4u * q.eb_plane_bytes;
const unsigned int eb_hop = x_total - (unsigned int) q.eb_step * (unsigned int)(CG * 4);
int f_within = rank - wgs_per_xcd, f_chunk = 0;
bool f_live = false;
const unsigned char *fa_base = nullptr, *fb_base = nullptr;
unsigned int fa_bytes = 0, fb_bytes = 0;
auto open_tile = [&] () {                             // next tile of this workgroup's list that holds outputs
    int st = 0, j0 = 0;
    f_live = false;
    for (f_within += wgs_per_xcd; f_within < tiles_per_xcd; f_within += wgs_per_xcd)
        if (tile_at (f_within, st, j0)) { f_live = true; break; }
    if (!f_live) return;
    const int la = max (i8_table_entry (tile_w0, 3 * st) + g.w_shift + j0 * g.Q + g.head_pad, 0);
    // the tile's exponent block and its first 4-frame block inside that block's own planes
    const int eb = j0 / q.eb_periods;
    unsigned int skip = (unsigned int) max ((la >> 2) - q.b0 - eb * q.eb_step, 0) * (unsigned int)(CG * 4);
    if (skip > q.eb_plane_bytes) skip = q.eb_plane_bytes;
    const size_t from = (size_t) eb * x_total + skip;
    fb_base = q.x_planes + from; fb_bytes = (unsigned int) min (q.x_bytes - from, (size_t) 0xfffffff0u);
#pragma unroll
    for (int u = 0; u < NB; ++u) bdel [u] = (unsigned int)((j0 + bper [u]) / q.eb_periods - eb) * eb_hop;
    fa_bytes = (unsigned int) nchunks * A_STEP;
    fa_base = q.a_planes + (size_t)(st * q.g + (j0 + q.jr_rot) % q.g) * fa_bytes;
};
#elif I8_PART == 3
// ---- matrix waves, in front of a tile's K loop (st, j0 = the tile; jl, c = the lane's period group and channel): exponent, accumulators, row masks

// rows carry 30 fraction bits, this lane's channel 2^shift in its period's exponent block; the class sums are combined at
// weight 256^(4 - s) in units of 2^16: the result is scaled by 2^(-14 - shift) (loaded now, used after the K loop)
const int out_exp = -14 - q.shifts [((j0 + jl * q.g) / q.eb_periods) * CG + c];
i32x16 acc [5];
#pragma unroll
for (int s = 0; s < 5; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc [s] [r] = 0;
// chunks in which some row of this tile has a non-zero most significant digit (the few around the rows' centres: taps
// fall off as 1 / distance): everywhere else the four products with that digit plane are exactly zero and not issued
// (and likewise the second digit plane — zero in the window's tails, where the taps are below 2^-15: its four products too)
unsigned long long top = q.a_masks [(st * q.g + (j0 + q.jr_rot) % q.g) * 32 + (lane & 31)], sec = q.a_masks [q.mask_words + (st * q.g + (j0 + q.jr_rot) % q.g) * 32 + (lane & 31)];
#pragma unroll
for (int off = 1; off < 32; off <<= 1) { top |= __shfl_xor (top, off); sec |= __shfl_xor (sec, off); }
const unsigned int top_lo = __builtin_amdgcn_readfirstlane ((unsigned int) top), top_hi = __builtin_amdgcn_readfirstlane ((unsigned int)(top >> 32));
const unsigned int sec_lo = __builtin_amdgcn_readfirstlane ((unsigned int) sec), sec_hi = __builtin_amdgcn_readfirstlane ((unsigned int)(sec >> 32));
#elif I8_PART == 4
// ---- matrix waves: the products of chunk ch (av, bv = the operands' four digit planes): the rows' two lower planes always, the second and the
// first where the masks have the chunk

#pragma unroll
for (int i = 2; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i + j <= 4) acc [i + j] = __builtin_amdgcn_mfma_i32_32x32x32_i8 (av [i], bv [j], acc [i + j], 0, 0, 0);
if (((ch < 32 ? sec_lo >> ch : sec_hi >> (ch - 32)) & 1u) != 0u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc [1 + j] = __builtin_amdgcn_mfma_i32_32x32x32_i8 (av [1], bv [j], acc [1 + j], 0, 0, 0);
}
if (((ch < 32 ? top_lo >> ch : top_hi >> (ch - 32)) & 1u) != 0u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc [j] = __builtin_amdgcn_mfma_i32_32x32x32_i8 (av [0], bv [j], acc [j], 0, 0, 0);
}
#elif I8_PART == 5
// ---- matrix waves: the tile's outputs (col_live: the lane's column exists — CG 1 and 2 may leave some unused; out_off: the lane's offset inside a tile).
// C/D layout of 32x32: row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), col = lane & 31
const unsigned int n_tile = a.n_begin + (unsigned int) j0 * g.P + (unsigned int)(st * 32);
const int rows_valid = min (32, g.P - st * 32);
const size_t left = (size_t)(a.n_end - n_tile) * CG * 4;
const __amdgpu_buffer_rsrc_t rs_out = make_rsrc (a.out + (size_t) n_tile * CG, left > 0xffffff00ull ? 0xffffff00u : (unsigned int) left);
const unsigned int pass_rows = PASS ? (unsigned int) g.tile_w0 [3 * st + 1] : 0u;
// (a launch on rows kept across calls starts mid-period: the slots of its first period in front of its first output are not stored.
// They sit in the first CG columns of the first matrix wave of the launch's first period group: a scalar bound — 0 everywhere else —
// and a test on the lane's own number, nothing kept live through the tile loop)
const int lo = a.n_skip != 0 && j0 == 0 && wave == 0 ? a.n_skip - st * 32 : 0;
// (the lane's half, opaque and per tile: as loop invariants the slot numbers below were computed in front of the tile loop, spilled and read back per tile)
int half = lane >> 5;
asm volatile ("" : "+v" (half));
#pragma unroll
for (int r = 0; r < 16; ++r) {
    const int i_const = (r & 3) + 8 * (r >> 2);      // compile-time part of the slot
    // class sums, weights 256^(4 - s), as one exact 64-bit integer, scaled back by the rows' and the channel's exponents (a
    // power of two: exact) and rounded ONCE to float — the same arithmetic in every fixed-point kernel: the same bits
    float y = i8_round (i8_total (acc [0] [r], acc [1] [r], acc [2] [r], acc [3] [r], acc [4] [r]), out_exp);
    const int i = i_const + 4 * half;
    if constexpr (PASS) {
        // nearest-filter mode, the position falls exactly on an input sample: the reference copies it (resampler.c:1141-1142)
        if ((pass_rows >> i) & 1u)
            y = load_frame (a, INT_MIN, g.canon_ip [st * 32 + i] + g.w_shift + g.canon_fi [st * 32 + i] / a.F + (j0 + jl * q.g) * g.Q, c);
    }
    if (col_live && i < rows_valid && (i >= lo || (lane & 31) >= CG))      // (frames at or past n_end: out of the resource's range, dropped)
        __builtin_amdgcn_raw_buffer_store_b32 (__float_as_uint (y), rs_out, (int)(out_off + (unsigned int)(i_const * CG) * 4u), 0, CG >= 8 ? ST_TILE32_OUT : 0);      // (measured at 8 channels only: narrower streams keep the default)
}
#endif
#undef I8_PART
