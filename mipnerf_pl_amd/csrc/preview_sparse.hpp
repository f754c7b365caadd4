// The storage rule of libmipnerf_preview_sparse.so (include/mipnerf_preview_sparse.h), stated ONCE.  MIP_HD like preview_march.hpp: the
// same source is inlined into k_preview_wave_march (preview_wave_march.hpp) and into the index kernels of kernels_preview_sparse.hip, and
// compiled with g++ by tests/hostmath/preview_sparse.cpp.  Integers only, apart from the blend, which is preview_march.hpp's.
//
// STORED POINTS.  A lattice point is stored iff any of the up to 8 cells around it is a STORED CELL, so every corner of a stored cell
// is stored.  The stored cells are the occupied cells of a single lattice; a level of a pyramid adds the cells in which a sample is
// read because its neighbouring level's cell is occupied (P5's OR; include/mipnerf_preview_sparse.h, preview.pyramid_storage).  The
// functions below take the stored cells' words `occ` where they build the table and never look at the march's occupancy words.
// Stored points are numbered in flat order (k * ny + j) * nx + i; the compact rows are fp16 [M, W], M = the number of stored points, W
// and the alignment as in mipnerf_preview.h.
// TABLE.  Per x-line (j, k) of POINTS, words_p = ceil(nx / 32) entries of two uint32, layout [nz, ny, words_p, 2]:
//     mask = the stored bits of points 32 w .. 32 w + 31 of the line (bit i & 31 of word i >> 5; bits at i >= nx are clear)
//     rank = the number of stored points before this word in flat order
// interleaved so that one 8-byte load serves a lookup: slot of point i = rank + popc(mask & ((1u << (i & 31)) - 1)).
// words_p is NOT the occupancy grid's words_x = ceil((nx - 1) / 32): they differ at nx = 32 m + 1.
// M < 2^31 follows from the lattice rule 7 nx ny nz < 2^31; a row's offset in bytes is formed in 64 bits.
#pragma once

#include "preview_mip.hpp"

namespace mip {

struct alignas(8) SparseEntry {      // one 8-byte load
    uint32_t mask, rank;
};

struct PreviewSparseField : PreviewField {      // `rows` is compact [M, W]; `occ` is never null
    const SparseEntry* table;                   // [nz, ny, words_p]
    int words_p;                                // ceil(nx / 32)
};

struct PreviewSparsePyramid {                   // PreviewPyramid (preview_mip.hpp) over sparse levels
    int levels;
    float spacing[kMipMaxLevels];
    PreviewSparseField level[kMipMaxLevels];
};

MIP_HD constexpr int sparse_words_p(int nx) { return (nx + 31) / 32; }
MIP_HD constexpr int sparse_words_x(int nx) { return (nx - 1 + 31) / 32; }

MIP_HD int sparse_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// the low `n` bits of a word, n <= 0 giving none and n >= 32 all
MIP_HD uint32_t sparse_low_bits(int n) { return n <= 0 ? 0u : n >= 32 ? 0xffffffffu : (1u << n) - 1u; }

// The stored bits of word w of the point line (j, k), from the cell words by word arithmetic.  Point i of a line is next to cells i - 1
// and i of the up to four cell lines (j - 1 .. j, k - 1 .. k) that exist: with c the cell word w (cells past nx - 2 masked off, as
// preview.occupied_cells slices them off) and p the cell word before it, the point bits are c | c << 1 | p >> 31, OR-ed over those lines.
MIP_HD uint32_t sparse_point_word(const uint32_t* occ, int nx, int ny, int nz, int j, int k, int w) {
    const int words_x = sparse_words_x(nx);
    uint32_t bits = 0u;
    for (int dk = -1; dk <= 0; ++dk)
        for (int dj = -1; dj <= 0; ++dj) {
            const int cj = j + dj, ck = k + dk;
            if (cj < 0 || cj > ny - 2 || ck < 0 || ck > nz - 2) continue;
            const uint32_t* line = occ + ((int64_t)ck * (ny - 1) + cj) * words_x;
            const uint32_t c = w < words_x ? line[w] & sparse_low_bits(nx - 1 - 32 * w) : 0u;
            const uint32_t p = w > 0 ? line[w - 1] & sparse_low_bits(nx - 1 - 32 * (w - 1)) : 0u;      // w - 1 < words_x: w < words_p
            bits |= c | (c << 1) | (p >> 31);
        }
    return bits & sparse_low_bits(nx - 32 * w);
}

// the slot of point i of a line whose entry of word i >> 5 is `e`; the point must be stored
MIP_HD int64_t sparse_slot(const SparseEntry& e, int i) { return (int64_t)e.rank + sparse_popc(e.mask & ((1u << (i & 31)) - 1u)); }

// rule 4's occupancy bit: the level's own occupancy words, as in the dense storage
MIP_HD bool preview_occupied(const PreviewSparseField& f, const int c[3]) {
    return preview_occupied(static_cast<const PreviewField&>(f), c);
}

// The compact storage's addresses, for a cell c the march reads (a STORED cell): its 8 corners are stored, so on each of its four
// x-lines the points c[0] and c[0] + 1 are both stored and nothing lies between them: the slot of corner c[0] + 1 is the slot of corner
// c[0] plus one, also when the two fall into different table words.  Four table loads, no straddling case; the blend reads row `slot`
// and the row after it.
template <int DEG>
MIP_HD void preview_row(const PreviewSparseField& f, const int c[3], const float fr[3], float (&row)[preview_row_halves(DEG)]) {
    constexpr int CH = PreviewRowChunks<DEG>::CH;
    typedef typename PreviewRowChunks<DEG>::Chunk Chunk;
    const SparseEntry* e = f.table + ((int64_t)c[2] * f.box.ny + c[1]) * f.words_p + (c[0] >> 5);
    const int64_t sy = f.words_p, sz = (int64_t)f.words_p * f.box.ny;     // in entries
    const SparseEntry e00 = e[0], e10 = e[sy], e01 = e[sz], e11 = e[sz + sy];
    const Chunk* q = reinterpret_cast<const Chunk*>(f.rows);
    preview_blend<DEG>(q + sparse_slot(e00, c[0]) * CH, q + sparse_slot(e10, c[0]) * CH, q + sparse_slot(e01, c[0]) * CH,
                       q + sparse_slot(e11, c[0]) * CH, fr, row);
}

}  // namespace mip
