/* mipnerf_preview_sparse.h -- C ABI of libmipnerf_preview_sparse.so: the baked preview over lattices that STORE ONLY THE ROWS THE MARCH
 * READS.  A fifth library: libmipnerf_preview.so (include/mipnerf_preview.h) keeps its 4 entry points, libmipnerf_preview_mip.so
 * (include/mipnerf_preview_mip.h) its 3 and the drop-in library (include/mipnerf_hip.h) its 93.
 *
 * Built by `python -m mipnerf_pl_amd.build` from csrc/kernels_preview_sparse.hip + csrc/preview_sparse_capi.hip; csrc/preview_sparse.hpp
 * states the storage rule once, for the device and for a host compiler, and takes everything else from csrc/preview_march.hpp and
 * csrc/preview_mip.hpp.  Conventions of mipnerf_preview.h: raw device pointers, the stream as void*, 0 = ok, 1 = invalid argument,
 * 2 = unsupported, 3 = HIP error, the message from the last-error call (thread-local); the library never allocates and never
 * synchronises, so every call can be captured into a hipGraph; every argument is validated before any HIP call.
 *
 * WHY NOTHING CHANGES IN THE PICTURE: a sample in a cell whose occupancy bit is clear loads no row (rule 4 of mipnerf_preview.h), so the
 * rows a march of ONE level reads are exactly the corners of occupied cells.  Storing those rows alone and marching with the rules of
 * mipnerf_preview.h gives the bytes the dense lattice with the same occupancy gives.  A level of a PYRAMID is read in more cells than
 * its own occupied ones: a sample between two levels is occupied when EITHER level's bit is set and then reads both (P5 of
 * mipnerf_preview_mip.h).  So the cells whose corners are stored -- the STORED CELLS, the words mipnerf_preview_sparse_index is given --
 * are a set of their own: the occupied cells for one level; for a level of a pyramid those plus every cell that shares a point with an
 * occupied cell of the level below or above (mipnerf_pl_amd.preview.pyramid_storage forms them).  More stored cells never change a
 * byte: the march reads the level's own occupancy words; the stored cells only decide which rows exist.
 *
 * STORAGE RULE (dims = (nx, ny, nz) points, flat index (k * ny + j) * nx + i, as in mipnerf_preview.h):
 * S1. A lattice point is STORED iff any of the up to 8 cells around it is a stored cell.  Every corner of a stored cell is
 *     stored.  Stored points are numbered in flat order: the SLOT of a stored point is the number of stored points before it.
 * S2. Rows.  fp16 [M, W], M = the number of stored points, row `slot` as the ROWS paragraph of mipnerf_preview.h states a row;
 *     16-byte aligned (8 for degree 0).  M < 2^31 follows from 7 nx ny nz < 2^31.
 * S3. Table.  uint32 [nz, ny, words_p, 2], words_p = ceil(nx / 32), 8-byte aligned: per x-line (j, k) of points and per word w
 *         mask = the stored bits of points 32 w .. 32 w + 31 of the line (point i = bit i & 31 of word i >> 5; bits at i >= nx clear)
 *         rank = the number of stored points before this word in flat order
 *     and slot(i) = rank + popcount(mask & ((1 << (i & 31)) - 1)).  words_p is not the occupancy grid's ceil((nx - 1) / 32).
 * S4. In a stored cell, corner i + 1 of an x-line is the next stored point after corner i, so its slot is slot(i) + 1, also across a
 *     word boundary: a sample makes 4 table loads, one per x-line of its cell.
 * THE TABLE AND THE OCCUPANCY MUST DESCRIBE THE SAME LATTICE: the table must be what mipnerf_preview_sparse_index writes for stored cells
 * that include every cell the march reads with the occupancy words it is given (above).  The march does not check this; with a table
 * of other bits it reads rows of other points or beyond the M rows. */
#ifndef MIPNERF_PREVIEW_SPARSE_H
#define MIPNERF_PREVIEW_SPARSE_H

#include <stddef.h>

#include "mipnerf_preview.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    mipnerf_preview_field_t field;    /* rows: compact fp16 [n_rows, W] (NULL only when n_rows == 0); occupancy: never NULL */
    const uint32_t* table;            /* [nz, ny, ceil(nx / 32), 2], 8-byte aligned */
    int64_t n_rows;                   /* M, 0 .. nx ny nz */
} mipnerf_preview_sparse_field_t;

typedef struct {
    int32_t levels;                               /* L, 1 .. 8 */
    mipnerf_preview_sparse_field_t level[8];      /* level[0] the finest; entries from L on are ignored */
} mipnerf_preview_sparse_pyramid_t;

int mipnerf_preview_sparse_abi_version(void);      /* 1 */
const char* mipnerf_preview_sparse_last_error(void);
/* bytes of the scan scratch mipnerf_preview_sparse_index needs for dims = (nx, ny, nz); 0 with the last error set when dims are invalid */
size_t mipnerf_preview_sparse_scratch_bytes(const int32_t* dims);
/* The table (S3) and the stored count of the stored cells' words [nz - 1, ny - 1, ceil((nx - 1) / 32)], in the layout of the occupancy
 * words and, for one level, the occupancy words themselves (never NULL: a lattice with every cell occupied gains nothing and stays
 * dense).  total: one device int32 that receives M; scratch: 4-byte aligned device memory of
 * mipnerf_preview_sparse_scratch_bytes(dims).  No atomics: two runs give the same bytes. */
int mipnerf_preview_sparse_index(const int32_t* dims, const uint32_t* occupancy, uint32_t* table, int32_t* total, void* scratch,
                                 void* stream);
/* rows[slot] = dense_rows[point] for every stored point, bytes copied; dense_rows fp16 [nz, ny, nx, W], rows fp16 [M, W]. */
int mipnerf_preview_sparse_gather(const int32_t* dims, int32_t degree, const uint32_t* table, const void* dense_rows, void* rows,
                                  void* stream);
/* rows [n_rows, W] from sigma fp32 [n_rows] and coef fp32 [n_rows, (degree + 1)^2, 3] of the stored points, in slot order, with the
 * rounding of mipnerf_preview_pack.  No mask: a stored point of one level is a baked point; a point a pyramid level stores beyond
 * those is handed zero coefficients, which pack to the zeros the mask writes.  n_rows == 0 is ok whatever the pointers. */
int mipnerf_preview_sparse_pack(int64_t n_rows, int32_t degree, const float* sigma, const float* coef, void* rows, void* stream);
/* mipnerf_preview_mip_march (rules P1 - P7 of mipnerf_preview_mip.h, its validation included) over sparse levels.  With one level, NULL
 * radii (every radius is 0) and footprint 0 it is mipnerf_preview_march.  origins / directions fp32 [n_rays, 3], radii (or NULL) / near /
 * far fp32 [n_rays]; rgb fp32 [n_rays, 3], acc / distance fp32 [n_rays]; steps int32 [n_rays] or NULL; lod fp32 [n_rays] or NULL.
 * n_rays == 0 is ok whatever the ray pointers. */
int mipnerf_preview_sparse_march(const mipnerf_preview_sparse_pyramid_t* pyramid, const mipnerf_preview_params_t* params, float footprint,
                                 int64_t n_rays, const float* origins, const float* directions, const float* radii, const float* near,
                                 const float* far, float* rgb, float* acc, float* distance, int32_t* steps, float* lod, void* stream);

#ifdef __cplusplus
}
#endif
#endif
