/* mikrylov.h -- C ABI of libmikrylov.so, the MI355X (gfx950) Krylov inner-loop engine.
 *
 * The reference (PythonOptimizers/pykrylov) is pure Python and has no FFI of its own;
 * its extension point is the duck-typed operator protocol `y = op * x`
 * (pykrylov/linop/linop.py:356-369) and the solver protocol
 * `Solver(op, **kw).solve(rhs, **kw)` (pykrylov/generic/generic.py:65-98).
 * Each entry point below names the reference code whose work it takes over.  The
 * Python package `pykrylov_amd` binds these with ctypes (INTEGRATION.md shows the
 * stub a reference maintainer would add).
 *
 * Conventions: every function returns 0 on success and a negative mk_status on
 * failure (text via mk_last_error()); no C++ exception crosses the boundary; all
 * "_dev" pointers are device (HBM) addresses obtained from mk_malloc; host arrays are
 * borrowed for the duration of the call only; one host thread per process drives one
 * device (one process per GPU).  Vectors are contiguous fp64, indices int32.
 */
#ifndef MIKRYLOV_H
#define MIKRYLOV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MK_VERSION 100

/* The library is built with -fvisibility=hidden: exactly the entry points declared here are exported (`nm -D`). */
#define MK_API __attribute__((visibility("default")))

typedef enum {
    MK_OK = 0,
    MK_ERR_HIP = -1,        /* a HIP runtime call failed (no GPU, OOM, launch failure) */
    MK_ERR_ARG = -2,        /* bad argument (null pointer, negative size, shape mismatch) */
    MK_ERR_STATE = -3,      /* call out of order (e.g. iterate before setup) */
    MK_ERR_COMM = -4,       /* RCCL failure or communicator missing */
    MK_ERR_UNSUPPORTED = -5
} mk_status;

/* ------------------------------------------------------------------ context ---- */
MK_API int mk_version(void);
/* Digest (16 hex digits) of the sources this binary was compiled from -- csrc/*.hip, csrc/*.h and this header, as
 * pykrylov_amd/build.py `source_sha()` computes it -- or "unknown" for a build made without build.py.  The Python package
 * refuses to load a library whose digest differs from its tree's (MIKRYLOV_ALLOW_STALE=1 overrides). */
MK_API const char *mk_build_info(void);
/* Bind the calling process to `device`, create the compute stream.  Idempotent. */
MK_API int mk_init(int device);
MK_API int mk_shutdown(void);
MK_API const char *mk_last_error(void);
/* name: at least 256 bytes.  Any out pointer may be NULL. */
MK_API int mk_device_info(char *name, int *compute_units, size_t *hbm_bytes);
MK_API int mk_sync(void);

/* ------------------------------------------------------------------ memory ----- */
MK_API int mk_malloc(void **dptr, size_t bytes);
MK_API int mk_free(void *dptr);
MK_API int mk_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
MK_API int mk_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
MK_API int mk_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes);
MK_API int mk_memset(void *dst_dev, int byte, size_t bytes);
/* Vector arena: ONE device allocation of `bytes` from which the solvers created afterwards carve their loop vectors
 * (2 MiB granules) instead of allocating each with hipMalloc; a solver that finds no room falls back to hipMalloc.
 * Meant to be called BEFORE a large matrix is built: how fast the fused update kernels stream depends on where the
 * vectors lie in HBM relative to each other, and a fresh device places them better than a device that
 * already holds 20 GB of matrix.  bytes = 0 releases the arena.  MK_ERR_STATE while vectors of it are in use. */
MK_API int mk_arena_reserve(size_t bytes);

/* Profiling aid: stream `bytes` of device memory with `width` (4, 8 or 16) bytes per lane, reading
 * (write = 0) or writing (write = 1).  Known byte counts to calibrate rocprofv3 FETCH_SIZE / WRITE_SIZE. */
MK_API int mk_calib_stream(void *dev, int64_t bytes, int width, int write);

/* Device vectors handed to this library (x, y, rhs, guess, preconditioner diagonals ...) must be 16-byte aligned and
 * readable up to an even number of entries (kernels move vectors in 16-byte pairs); every buffer from mk_malloc is.
 * Misaligned pointers are rejected with MK_ERR_ARG. */

/* ------------------------------------------------------------------ CSR -------- */
/* The device-resident operator behind `linop.LinearOperator`: replaces the user
 * `matvec` callable of pykrylov/linop/linop.py:114,:289 (Pysparse in
 * examples/demo_common.py:15-16).  Canonical CSR: sorted columns, no duplicates. */
typedef struct mk_csr mk_csr;

MK_API int mk_csr_create(int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *indptr_host,
                  const int32_t *indices_host, const double *data_host, mk_csr **out);
MK_API int mk_csr_destroy(mk_csr *A);
MK_API int mk_csr_shape(const mk_csr *A, int64_t *nrows, int64_t *ncols, int64_t *nnz);
/* Smallest and largest stored column index (2147483647 / -1 without entries), found on the device: the range check
 * a binding applies to a matrix built from caller arrays (the reference has none: its operator wraps a callable,
 * linop/linop.py:114; an out-of-range column would read outside x). */
MK_API int mk_csr_col_range(const mk_csr *A, int32_t *min_col, int32_t *max_col);
/* Canonical CSR from coordinate triples (host arrays, borrowed), built on the device: the on-disk side of the
 * path -- MatrixMarket coordinate files (examples/1138bus.mtx, jpwh_991.mtx; examples/demo_common.py:12-16 used
 * Pysparse for this) and the reference's CoordLinearOperator (linop.py:638-685).  Columns sorted per row,
 * duplicate entries summed in input order starting from 0.0 (the result of a stable host sort + np.add.at):
 * integer arrays and values are bit-identical to that host construction.  Symmetric storage must be mirrored by
 * the caller.  MK_ERR_UNSUPPORTED if one row holds more than 16384 entries (use mk_csr_create then). */
MK_API int mk_csr_from_coo(int64_t nrows, int64_t ncols, int64_t nentries, const int32_t *rows_host,
                    const int32_t *cols_host, const double *vals_host, mk_csr **out);
/* Copy the arrays back (any pointer may be NULL). */
MK_API int mk_csr_download(const mk_csr *A, int32_t *indptr_host, int32_t *indices_host, double *data_host);
/* The same for the rows [row_begin, row_end) only: indptr_host receives row_end - row_begin + 1 row pointers AS STORED
 * (offsets into the whole matrix: subtract the first to index the slices), indices_host / data_host the entries
 * indptr[row_begin] .. indptr[row_end).  Call once with NULL arrays for the row pointers to learn the sizes.  This is
 * how a 512^3 matrix (11.8 GB of arrays) is checked against the oracle slab by slab (tests/test_gpu_full_size.py). */
MK_API int mk_csr_download_rows(const mk_csr *A, int64_t row_begin, int64_t row_end, int32_t *indptr_host,
                         int32_t *indices_host, double *data_host);
/* B = A^T as a new canonical CSR built on the device (operator `.T`, linop.py:148-171;
 * feeds `A.T * u` of pykrylov/lls/lsqr.py:200,264). */
MK_API int mk_csr_transpose(const mk_csr *A, mk_csr **out);
/* Synthetic matrices generated directly in HBM.  Rows
 * [row_begin,row_end) of the global matrix, global column ids.
 * poisson2d: 5-point, m x m grid (the matrix of pykrylov/gallery/gallery.py:10-29).
 * poisson3d: 7-point, nx x ny x nz grid, x fastest. */
MK_API int mk_csr_poisson2d(int64_t m, int64_t row_begin, int64_t row_end, mk_csr **out);
MK_API int mk_csr_poisson3d(int64_t nx, int64_t ny, int64_t nz, int64_t row_begin, int64_t row_end, mk_csr **out);
/* poisson3d_varcoef: -div(k grad u) on the same grid with the same sparsity (integer arrays identical to poisson3d),
 * k a positive cell field hashed from `seed`; entries are minus the harmonic means of neighbouring cells, the diagonal
 * their sum plus k itself per missing neighbour (Dirichlet).  SPD, practically all stored values distinct: the workload
 * on which no constant-coefficient compression applies (bench.py `poisson3d-512-varcoef`; the matrix class a user's
 * `matvec` brings to linop/linop.py:271-298). */
MK_API int mk_csr_poisson3d_varcoef(int64_t nx, int64_t ny, int64_t nz, uint64_t seed, int64_t row_begin, int64_t row_end,
                             mk_csr **out);
/* stencil27: the 27-point box stencil on the same grid (HPCG's sparsity; rows of 8 ... 27 entries, columns ascending).
 * seed == 0: -1.0 off the diagonal, 26.0 on it; seed != 0: harmonic means of the hashed cell field as above, the
 * diagonal their left-to-right sum over the 26 directions (k itself per missing neighbour).  SPD.  No reference
 * counterpart beyond "a user's matvec" (linop/linop.py:271-298): the test matrix of the wide storage formats. */
MK_API int mk_csr_stencil27(int64_t nx, int64_t ny, int64_t nz, uint64_t seed, int64_t row_begin, int64_t row_end, mk_csr **out);

/* Operator algebra that stays on the device (linop.py:307-330 `alpha * op`, :375-398 `op + other`, :403-426
 * `op - other`, :400-401 `-op`, with `other` a DiagonalOperator (:473-516), an IdentityOperator (:455-470) or a scalar
 * multiple of one).  The reference evaluates such operators as `alpha * (op * x)`, `(op * x) + (other * x)`, ... one
 * NumPy expression per node; mk_csr_compose makes an operator that shares A's arrays (A must outlive it) and applies
 * the same expressions, in the same order, to every row sum before anything else sees it:
 *     t = (A x)_r ; for each step:   term = x_r ; if diag: term = diag[r] * term ; if has_scale: term = scale * term
 *        MK_ROW_SCALE  t = scale * t      MK_ROW_ADD  t = t + term      MK_ROW_SUB  t = t - term      MK_ROW_RSUB  t = term - t
 * Steps of A itself (if it is a composed operator) run first.  Square matrices only when a step uses x_r.
 * Every product of the library (mk_spmv and all solver kernels) honours the steps. */
enum { MK_ROW_SCALE = 1, MK_ROW_ADD = 2, MK_ROW_SUB = 3, MK_ROW_RSUB = 4, MK_ROWPROG_MAX = 4 };
typedef struct mk_rowop {
    int32_t code;         /* MK_ROW_* */
    int32_t has_scale;    /* term is multiplied by `scale` (always 1 for MK_ROW_SCALE) */
    double scale;
    const double *diag;   /* device array, nrows entries, borrowed; NULL: identity */
} mk_rowop;
MK_API int mk_csr_compose(const mk_csr *A, int32_t nops, const mk_rowop *ops, mk_csr **out);

/* Sum, difference and product of two device matrices as ONE device operator (linop.py:375-398 `op + other`, :403-426
 * `op - other`, :332-354 `op * other`): the reference evaluates them as `(A*x) + (B*x)`, `(A*x) - (B*x)` and `A*(B*x)`
 * -- two complete products and one element-wise operation -- and so does the device: the first product's row sums go
 * to a temporary, the second product's kernel combines them with its own row sums (or multiplies the temporary)
 * and feeds the result to the fused epilogue of whatever solver kernel asked for the product.  Same bits as the
 * reference's closures.  A and B are borrowed (destroying one while the result is alive is deferred until the result is destroyed); they may carry a row program
 * (mk_csr_compose) but must not be composites, matrix-free or partitioned.  sign = +1 / -1. */
MK_API int mk_csr_create_sum(const mk_csr *A, const mk_csr *B, int sign, mk_csr **out);
MK_API int mk_csr_create_product(const mk_csr *A, const mk_csr *B, mk_csr **out);

/* Restriction of a device matrix to the rows `rows` and columns `cols` (host index arrays, copied), as one device
 * operator: reference ReducedLinearOperator / SymmetricallyReducedLinearOperator (linop/linop.py:560-623), evaluated
 * the same way -- `z = 0; z[cols] = x; y = (A z)[rows]` -- with scatter, product and gather on the device.  `cols` must
 * not repeat an index.  A is borrowed (see mk_csr_create_sum). */
MK_API int mk_csr_create_reduced(const mk_csr *A, int64_t nrows, const int32_t *rows, int64_t ncols, const int32_t *cols,
                          mk_csr **out);

/* A grid of device matrices as ONE operator (reference linop/blkop.py:8-152 BlockLinearOperator, :154-257
 * BlockDiagonalLinearOperator): `blocks` lists nbr x nbc handles row by row (NULL = zero block), block (i, j) being
 * heights[i] x widths[j].  A product evaluates every block product completely and adds the results to the block row's
 * accumulator one block at a time, starting from +0.0 -- the reference's `y_i += B_ij * x_j` (blkop.py:86-96) -- so
 * results carry the same roundings, and the operator is accepted wherever a device matrix is (solver product sites
 * with their fused epilogues included).  The blocks are borrowed: destroying one while the block operator is alive is
 * deferred until the block operator is destroyed.  Device matrices with or without a row program; not composites. */
MK_API int mk_csr_create_block(int32_t nbr, int32_t nbc, const mk_csr *const *blocks, const int64_t *heights,
                        const int64_t *widths, mk_csr **out);
/* Matrix-free operator: the products of the returned handle are computed by a HOST callback -- the reference's own
 * operator protocol, `LinearOperator(nargin, nargout, matvec=callable)` (linop/linop.py:114,271-298), e.g. the gallery
 * operators its CG test runs on (cg/tests/test_diagdom.py:38-40).  Everything else of a solver loop (dots, updates,
 * scalar recurrences, stopping tests) still runs on the device: at each product site the loop's input vector is
 * materialised on the device, copied to the host, `fn(user, transpose, x_host, y_host)` is called (x_host: ncols
 * entries, or nrows when transpose != 0; return 0 on success), and the result feeds the same fused epilogue kernel
 * a CSR product would have fed.  The callback is invoked exactly when the reference would have invoked `op * v`
 * (never after the loop condition failed).  Single GPU only. */
typedef int (*mk_matvec_fn)(void *user, int transpose, const double *x_host, double *y_host);
MK_API int mk_csr_create_callback(int64_t nrows, int64_t ncols, mk_matvec_fn fn, void *user, int transpose, mk_csr **out);

/* Storage format the products of A stream from HBM, chosen per matrix and built on the device at the first product
 * (an acceleration structure beside the CSR arrays; results are bit-identical in every format):
 *   0  plain CSR: 4-byte columns + 8-byte values, x gathered through L1/L2;
 *   1  windowed tiles: per 256-row tile the referenced columns are covered by contiguous windows of x that the kernel
 *      stages in LDS with coalesced loads; per nonzero a uint16 LDS slot replaces the column (2 + 8 bytes);
 *   2  format 1 + value dictionary: matrices with <= 256 distinct values store ONE 32-bit word per nonzero
 *      {LDS slot : 16 | dictionary index : 8} and no values (4 bytes); slots, words and windows go to LDS by direct copies;
 *   4  format 2 + row patterns: when the rows of the windowed tiles follow <= 256 distinct sequences of
 *      {LDS slot - lane, dictionary index} words (stencils), ONE BYTE per row names its sequence and nothing is read
 *      per nonzero;
 *   5  format 1's windows + row patterns for matrices WITHOUT a dictionary (variable-coefficient stencils): one byte
 *      per row names its sequence of LDS slots, the values are streamed in tile-sliced ELL order (8 bytes per nonzero);
 *   6, 7, 8  the wide twins for rows of up to 32 entries (tiles of up to 8192 nonzeros in 32 window chunks), chosen when
 *      the cover of formats 1 .. 5 (16 chunks, 2048 nonzeros) reaches less than half of the tiles: 8 = dictionary + row
 *      patterns (one byte per row), 7 = row patterns + streamed values, 6 = uint16 slots + values both streamed in
 *      tile-sliced ELL order (10 bytes per nonzero; needs neither patterns nor a dictionary).  6 or 7 asked for
 *      explicitly are also applied to matrices formats 1 .. 5 would have served;
 *   3  plain CSR for matrices without a window cover whose x is longer than an L2: the tile's stream is held in LDS
 *      and the gathers of all workgroups walk x slice by slice (same arrays as format 0);
 *   9  z-marching bricks for 7-point-class matrices: every column offset in {0, +-1, +-L, +-P}, nrows % P == 0 (the 7-point
 *      stencil of ANY nx x ny x nz grid, L = nx, P = nx ny, any boundary treatment; any band matrix of that shape; a 5-point
 *      matrix with one far stride M as L = 128, P = M) and <= 256 distinct values: ONE BYTE per row names its pattern
 *      {7 values, presence mask}; a workgroup owns a brick of 4 lines x 128 rows and marches through the planes with the
 *      planes z-1, z, z+1 of its own rows in registers, so that every x entry is loaded once per product (format 4
 *      requests each five times).  Round 6: lines that are no multiple of 128 rows, planes that are no multiple of four
 *      lines and odd strides are served by general-geometry kernels whose partly empty bricks discard the rows that do not
 *      exist (mk_csr_march_info); at least half of the bricks' lanes must have rows.  General-geometry kernels exist for
 *      plain products and CG; any other loop on such a matrix runs the CSR gather kernel on the same arrays (same row sums
 *      bit for bit; its fused dots then follow tile order 0 over the march's grid, not the brick order).  Chosen
 *      AUTOMATICALLY from 2^21 rows on (MK_PENCIL_MIN_ROWS) where the bricks are at least 90 % full, from 2^24 rows on
 *      where they are 50 .. 90 % full, for 5-point matrices from 2^23 rows on -- where it was measured to win
 *      (profiles/r06_march_sizes.txt) --, and only while the last solver created on the matrix is CG or none; asked for
 *      explicitly it is applied to any matrix of the class.  Matrices outside the class degrade to 8 and below.
 *  10  format 9's march for matrices of the class WITHOUT a value dictionary (variable-coefficient stencils): the byte per
 *      row is its 7-bit presence mask and the values are streamed from seven position-major arrays (56 bytes per row,
 *      +0.0 where a row has no entry) -- what format 5 streams, with every x entry loaded once.  Chosen automatically
 *      (same size rule) when format 9 finds more than 256 values or patterns; asked for explicitly on any matrix of the class.
 *      Formats 9 .. 11 also serve ONE RANK'S SLAB of such a matrix -- whole planes, columns localised by mk_csr_localize
 *      mode 0, halo exchange -- taking the neighbours' planes from the received entries.
 *  11  format 10 for matrices that are SYMMETRIC bit for bit (what CG runs on): only the diagonal and the three upper values
 *      of a row are stored and streamed (32 bytes per row); the lower ones are the neighbouring rows' upper values, which
 *      the march has in registers (plane below) or passes through an LDS image of the plane's values (row before, line
 *      below).  The builder verifies the symmetry entry by entry; a matrix that is not symmetric stays format 10.
 * fmt = -1 restores the default (environment MK_SPMV_FORMAT, else 11 = the most compact format the matrix qualifies for;
 * format 3 is chosen automatically for scattered matrices with more than 5 MiB of x).  A request is an upper bound and
 * degrades silently (11 -> 10, 10 -> 9 -> 8, 8 -> 7 -> 6 -> 0, 5 -> 1, 4 -> 2 -> 1 -> 0, 3 -> 0): tiles with scattered columns always take the
 * gather path of format 0.
 * mk_csr_format_info reports what is in use: the format, the number of windowed tiles, the LDS chunks (128
 * doubles each) a workgroup reserves (format 3: the number of column phases), the dictionary size and the bytes of
 * matrix data (everything except x and y) one product streams (a format 9 matrix with z-uniform pattern bytes,
 * mk_csr_march_info [12]: three planes of bytes and the pattern table, not one byte per row). */
MK_API int mk_csr_set_format(mk_csr *A, int fmt);
MK_API int mk_csr_format_info(const mk_csr *A, int32_t *fmt, int64_t *tiles_windowed, int32_t *lds_chunks,
                       int32_t *dict_size, int64_t *matrix_bytes_per_product);
/* Column blocks: a plain-CSR matrix (format 0) can additionally be stored as K <= 16 column blocks of block_kb KiB of x
 * each (a second copy of the CSR data); its products then run block after block with the running row sums carried from one
 * launch to the next -- the same left-to-right sum, same bits -- every block a resident tile of format 3 with column phases
 * over its own slice of x, which fits an XCD's L2.
 * AUTOMATIC since round 4 (block_kb = -1, the state of a new matrix): on for long-row operators -- >= 12 entries per row on
 * average gathered from an x of >= 16 MB, e.g. the transpose of a tall least-squares matrix -- with 8 MiB blocks (4 MiB if a
 * block's tile outgrows the LDS budget), PROVIDED that x fits 16 blocks, the second copy fits a quarter of the free device
 * memory and every block's tiles are LDS resident; otherwise the matrix keeps its single launch.  The environment
 * variable MK_COLBLOCK_KB overrides the automatic choice (0 = never).  On 5-entry rows the single launch of format 3 is
 * faster, which is why short-row matrices are never blocked automatically.
 * block_kb > 0 forces blocks of that size for A, 0 turns them off.  mk_csr_colblocks reports K (0: not blocked). */
MK_API int mk_csr_set_colblocks(mk_csr *A, int32_t block_kb);
/* Tile order of the SpMV launches (speed only; it also fixes which rows a workgroup's partial sums of a fused dot
 * cover): 0 round robin, 1 each XCD sweeps its own contiguous eighth, 2 every step of the grid is cut into eight
 * XCD-contiguous blocks, 3 stripes of `stripe` tiles dealt round-robin to the XCDs, 4 as 3 but an XCD walks its strip
 * through all planes (`plane` tiles apart) before it takes its next strip; -1 = library default.  `nontemporal`: matrix
 * data that is read once per product, and the product vector of the CG loop, go past the caches (1 / 0 / -1 = default:
 * on when a vector is larger than the 256 MiB Infinity Cache).  mk_csr_tile_order reports what a launch would use now. */
MK_API int mk_csr_set_tile_order(mk_csr *A, int32_t order, int32_t stripe, int32_t plane, int32_t nontemporal);
MK_API int mk_csr_tile_order(const mk_csr *A, int32_t *order, int32_t *stripe, int32_t *plane, int32_t *nontemporal);
MK_API int mk_csr_colblocks(const mk_csr *A, int32_t *nblocks);
/* Launch geometry of A's product kernels (what fixes the summation order of the dots fused into them): the grid,
 * and the tile order (0 round robin; 1 each XCD sweeps a contiguous eighth; 2 XCD-contiguous blocks per step). */
MK_API int mk_csr_launch_info(const mk_csr *A, int32_t *grid, int32_t *tile_map);
/* Geometry of formats 9 / 10 (all zero when A is in another format): the line and plane strides L and P found in the matrix,
 * the number of planes, the planes a workgroup marches through per (brick, chunk) item, the chunks per brick and the
 * number of distinct row patterns.  Workgroup b of a launch of `grid` workgroups takes the items b, b + grid, ...;
 * item i = brick (i % bricks_per_plane) of chunk (i / bricks_per_plane) -- dealt XCD-contiguously when bricks_per_plane and
 * the grid are multiples of 8: brick (i % 8) bpp / 8 + (i / 8) % (bpp / 8) of chunk (i / 8) / (bpp / 8) --,
 * bricks_per_plane = bpp = (L / 128) (P / 4L), brick j
 * starting at row (j / (L / 128)) 4L + (j % (L / 128)) 128 of a plane -- what oracle/gpu_order.py restates for the
 * fused dots (test infrastructure). */
MK_API int mk_csr_pencil_info(const mk_csr *A, int64_t *stride_line, int64_t *stride_plane, int32_t *planes,
                              int32_t *planes_per_chunk, int32_t *chunks, int32_t *patterns);
/* The same and the rest of the brick geometry as an array (round 6: any grid side; all zero when A is in another format):
 *   info[0] storage format (9 / 10 / 11)      [1] L, line stride            [2] P, plane stride         [3] planes
 *   [4] lines per plane = ceil(P / L)          [5] bricks per line = ceil(L / 128)                       [6] brick rows = ceil(lines / 4)
 *   [7] planes per chunk                       [8] chunks                    [9] 2 = general geometry (partly empty bricks, pairs
 *   at any 8-byte boundary: a lane whose row does not exist -- in-line position >= L or in-plane index >= P -- discards its
 *   row sum), 0 = whole aligned bricks          [10] per: bricks per XCD of the XCD-contiguous deal, 0 = round robin
 *   [11] row patterns (format 9)               [12] 1 = z-uniform pattern bytes: every interior plane (1 .. planes - 2) carries
 *   the bytes of plane 1 (checked on the bytes when the format is built, planes >= 3) and the march reads them there -- one
 *   plane that stays in L2 instead of one byte per row from HBM in every product; the product's bits are the same.
 * Item i of a launch whose grid is a multiple of 8 with per > 0: brick (i % 8) per + (i / 8) % per of chunk (i / 8) / per
 * (8 per item slots per chunk; a slot whose brick number is >= bricks per plane is empty); otherwise brick i % bpp of
 * chunk i / bpp.  Brick j starts at row (j / bx) 4L + (j % bx) 128 of a plane.  A 5-point matrix (one far stride M) is
 * reported as L = 128, P = M: it is marched line by line.  At most `cap` entries are written (MK_MARCH_INFO_LEN exist). */
#define MK_MARCH_INFO_LEN 13
MK_API int mk_csr_march_info(const mk_csr *A, int64_t *info, int32_t cap);

/* y = A x   (K1; `self.op * p`, pykrylov/cg/cg.py:115 and every other solver).
 * x_dev must be 16-byte aligned and readable ONE ENTRY PAST ITS END (the kernels read pairs; a pair may start at the last
 * entry when a plane stride of the brick-march formats is odd): every buffer from mk_malloc has 16 bytes of slack.
 * Per row the products are added left to right with one rounding per multiply and per
 * add, so the result is bit-identical to a scalar CSR loop. */
MK_API int mk_spmv(const mk_csr *A, const double *x_dev, double *y_dev);

/* ------------------------------------------------------------------ BLAS-1 ----- */
/* K2/K3/K4 of SURVEY.md section 2.2: np.dot / np.linalg.norm / in-place updates of the
 * solver loops (e.g. pykrylov/cg/cg.py:117,130-131,146,150-151).  Deterministic
 * fixed-tree reductions; results returned to the host. */
MK_API int mk_dot(int64_t n, const double *x_dev, const double *y_dev, double *result_host);
MK_API int mk_nrm2(int64_t n, const double *x_dev, double *result_host);
MK_API int mk_axpy(int64_t n, double alpha, const double *x_dev, double *y_dev);               /* y += alpha*x   */
MK_API int mk_axpby(int64_t n, double alpha, const double *x_dev, double beta, double *y_dev); /* y = alpha*x + beta*y */
MK_API int mk_scal(int64_t n, double alpha, double *x_dev);                                    /* x *= alpha     */

/* ------------------------------------------------------------------ comm ------- */
/* Row-partitioned multi-GPU execution (one process per GPU, RCCL over xGMI).
 * unique_id: 128 bytes from mk_comm_unique_id on rank 0, broadcast by the caller. */
MK_API int mk_comm_unique_id(void *id128);
MK_API int mk_comm_init(int nranks, int rank, const void *id128);
/* Host-staged transport: the same collectives carried by caller-supplied functions on HOST buffers (for instance
 * torch.distributed with the gloo backend).  Every collective stages through pinned memory and synchronises the
 * stream: meant for exercising the multi-rank logic where RCCL cannot be used (several ranks on one GPU, CI), not
 * for speed.  Callbacks return 0 on success.
 *   allreduce(buf, count)                       in-place sum over all ranks
 *   exchange(send, send_count, send_off, recv, recv_count, recv_off)
 *                                               rank r gets send[send_off[r] .. +send_count[r]) and delivers
 *                                               recv_count[r] entries to recv + recv_off[r] (arrays of nranks)
 *   allgather(send, count, recv)                recv = concatenation over ranks of `count` entries each */
typedef int (*mk_host_allreduce_fn)(double *buf, int64_t count);
typedef int (*mk_host_exchange_fn)(const double *send, const int64_t *send_count, const int64_t *send_off,
                                   double *recv, const int64_t *recv_count, const int64_t *recv_off);
typedef int (*mk_host_allgather_fn)(const double *send, int64_t count, double *recv);
MK_API int mk_comm_init_host(int nranks, int rank, mk_host_allreduce_fn allreduce, mk_host_exchange_fn exchange,
                      mk_host_allgather_fn allgather);
MK_API int mk_comm_destroy(void);
MK_API int mk_comm_info(int *nranks, int *rank);
/* Which transport carries the collectives: *kind = 0 none, 1 RCCL, 2 host-staged callbacks; *rccl_ranks = what
 * ncclCommCount reports for the communicator (0 without RCCL) -- bench.py prints it so that a host-staged fallback can
 * never be mistaken for an RCCL measurement; *halo_comm_split = 1 if the halo messages have their own communicator. */
MK_API int mk_comm_transport(int *kind, int *rccl_ranks, int *halo_comm_split);
/* Attach an exchange plan to a local matrix whose columns are already remapped to
 * [local rows | halo]: before each SpMV the `send_count[r]` entries `send_idx`
 * (local indices, grouped by destination rank) go to rank r and `recv_count[r]` entries
 * arrive into the halo region in rank order.  mode 0 = halo send/recv, 1 = allgather
 * (then the matrix keeps global column ids and every rank owns `n_local` rows, the
 * last rank possibly fewer). */
MK_API int mk_csr_set_exchange(mk_csr *A, int mode, int64_t n_local, int64_t n_halo, const int64_t *send_count,
                        const int64_t *recv_count, const int32_t *send_idx_host);
/* Rewrite the global column ids of a row block [col_begin, col_end) of a square matrix into the
 * local numbering, in place, on the device.
 * mode 0 (halo): columns outside the owned range must lie in two contiguous windows next to it
 *   (banded / stencil matrices); their widths are returned in halo_lo / halo_hi and the new
 *   numbering is [owned | lower window | upper window], ncols becomes n_local + lo + hi.
 * mode 1 (allgather): col' = n_local + col, ncols becomes n_local + gathered_len. */
MK_API int mk_csr_localize(mk_csr *A, int mode, int64_t col_begin, int64_t col_end, int64_t gathered_len,
                    int64_t *halo_lo, int64_t *halo_hi);
/* x_ext_dev has n_local + n_halo entries: the rank's own slice first, received entries after. */
MK_API int mk_exchange(const mk_csr *A, double *x_ext_dev);
/* Sum `count` (<= 2048) host doubles over all ranks, in place; a no-op without a communicator.  For the few
 * reductions the host side of a partitioned run needs (e.g. tools.check_symmetric, utils.py:63-85). */
MK_API int mk_comm_allreduce_host(double *vals_host, int64_t count);
/* Timing aids (collective: every rank calls them with the same arguments in the same order).  Average duration
 * in microseconds of `reps` back-to-back in-stream exchanges of A's plan (halo: pack + grouped send/recv; all-gather)
 * resp. all-reduces of `count` (<= 2048) doubles, bracketed by one HIP event pair on the library stream. */
MK_API int mk_comm_time_exchange(const mk_csr *A, double *x_ext_dev, int64_t reps, double *avg_us);
MK_API int mk_comm_time_allreduce(int64_t count, int64_t reps, double *avg_us);
/* Duration of the last overlapped halo message group on the second stream (0: none yet). */
MK_API int mk_csr_comm_last_us(const mk_csr *A, double *us);
/* Halo mode overlaps the messages with the product: tiles (256 rows) whose rows reference only owned columns are
 * multiplied while the neighbours' entries travel on a second stream, the remaining tiles afterwards.  Reports the
 * split (0, 0: no overlap plan -- single rank, all-gather mode, or every tile touches the halo). */
MK_API int mk_csr_overlap_info(const mk_csr *A, int64_t *n_interior_tiles, int64_t *n_boundary_tiles);

/* ------------------------------------------------------------------ solvers ---- */
typedef enum {
    MK_CG = 1,        /* pykrylov/cg/cg.py:46-165            */
    MK_BICGSTAB = 2,  /* pykrylov/bicgstab/bicgstab.py:43-151 */
    MK_CGS = 3,       /* pykrylov/cgs/cgs.py:40-123           */
    MK_TFQMR = 4,     /* pykrylov/tfqmr/tfqmr.py:39-159       */
    MK_MINRES = 5,    /* pykrylov/minres/minres.py:115-410    */
    MK_SYMMLQ = 6,    /* pykrylov/symmlq/symmlq.py:65-400     */
    MK_LSQR = 7,      /* pykrylov/lls/lsqr.py:86-453          */
    MK_LSMR = 8,      /* pykrylov/lls/lsmr.py:64-492          */
    MK_CRAIG = 9,     /* pykrylov/lls/craig.py:104-520        */
    MK_CRAIGMR = 10,  /* pykrylov/lls/craigmr.py:51-241       */
    MK_GMRES = 11,    /* restarted GMRES(m), right preconditioned (no reference module): a square solver */
    MK_IDR = 12,      /* IDR(s), right preconditioned (no reference module): a square solver */
    MK_PCG = 13,      /* preconditioned CG, the textbook recurrence p = z + beta p (no reference module): a square solver */
    MK_MSCG = 14,     /* multi-shift CG: (A + sigma_k I) x_k = b for up to MK_MSCG_MAX_SHIFTS shifts in one Krylov space (no reference module): a square solver */
    MK_TRLAN = 15,    /* thick-restart Lanczos (Wu and Simon): the nev smallest or largest eigenpairs of a symmetric operator (no reference module); not a solver of A x = b */
    MK_LOBPCG = 16,   /* LOBPCG (Knyazev): a block, preconditioned eigensolver with soft locking for the nev smallest or largest eigenpairs of a symmetric operator (no reference module); not a solver of A x = b */
    MK_TRSVD = 17     /* thick-restart Golub-Kahan-Lanczos bidiagonalisation (Baglama and Reichel): the nev largest or smallest singular triplets of a tall operator; needs mk_solver_set_transpose (no reference module); not a solver of A x = b */
} mk_solver_kind;

#define MK_GMRES_MAX_RESTART 128
#define MK_IDR_MAX_S 32
#define MK_MSCG_MAX_SHIFTS 32
#define MK_TRLAN_MAX_NCV 128
#define MK_LOBPCG_MAX_BLOCK 16

typedef struct {
    int32_t struct_size;      /* = sizeof(mk_params), or sizeof(mk_params_shifts) / sizeof(mk_params_eig) at the head of a long block below */
    int32_t kind;             /* mk_solver_kind */
    double abstol;            /* generic.py:74 */
    double reltol;            /* generic.py:75 */
    int64_t matvec_max;       /* cg.py:82 (default 2n is applied by the caller) */
    int32_t check_curvature;  /* cg.py:67 */
    int32_t has_shift;        /* symmlq.py:92-93: shift None vs value */
    double shift;             /* minres.py:122, symmlq.py:92 */
    double rtol;              /* minres.py:126, symmlq.py:90 */
    double etol;              /* minres.py:127 */
    int64_t itnlim;           /* minres.py:125 */
    int32_t window;           /* minres.py:130 */
    int32_t spmv_event_stride; /* >0: bracket the SpMV kernel of every k-th pass with HIP events */
    double damp;              /* lsqr.py:86, lsmr.py:64 */
    double atol;              /* lsqr.py:86 */
    double btol;              /* lsqr.py:86 */
    double conlim;            /* lsqr.py:87 */
    int32_t restart;          /* MK_GMRES: steps per cycle, 1 .. MK_GMRES_MAX_RESTART (clamped to n); MK_ERR_ARG otherwise */
    int32_t reorth;           /* MK_GMRES: 1 = classical Gram-Schmidt twice per step, 0 = once; MK_TRSVD: 1 = both bases are orthogonalised in full, 0 = the V basis only (one-sided); MK_ERR_ARG otherwise */
} mk_params;

/* The long parameter block: mk_params followed by the shifts of MK_MSCG.  mk_params itself is unchanged, so that callers
 * compiled against it keep working; mk_solver_create tells the two apart by struct_size.  Hand it `&block.base` with
 * block.base.struct_size = sizeof(mk_params_shifts).  Every solver kind accepts either block, only MK_MSCG reads the
 * tail, and MK_MSCG refuses the short block (MK_ERR_ARG: it has no shifts). */
typedef struct {
    mk_params base;
    int32_t nsigma;           /* number of shifts, 1 .. MK_MSCG_MAX_SHIFTS; MK_ERR_ARG otherwise */
    int32_t sigma_reserved;   /* (padding; ignored) */
    double sigma[MK_MSCG_MAX_SHIFTS];   /* the shifts sigma_k, k < nsigma, each finite */
} mk_params_shifts;

/* The second long parameter block: mk_params followed by what the eigensolvers MK_TRLAN and MK_LOBPCG (and MK_TRSVD) ask for.  It is told
 * apart by struct_size like the first: hand mk_solver_create `&block.base` with block.base.struct_size =
 * sizeof(mk_params_eig).  Every solver kind accepts it, only MK_TRLAN and MK_LOBPCG read the tail, and both refuse the other
 * two blocks (MK_ERR_ARG).  MK_TRLAN: MK_ERR_ARG unless 1 <= nev < ncv <= min(n, MK_TRLAN_MAX_NCV) and, for a keep that is
 * not 0, nev <= keep < ncv.  MK_LOBPCG: `ncv` carries the block size nb, MK_ERR_ARG unless
 * 1 <= nev <= nb <= min(MK_LOBPCG_MAX_BLOCK, n / 3) and keep == 0.  MK_TRSVD reads the tail as MK_TRLAN does, nev being the
 * singular triplets wanted: MK_ERR_ARG unless 1 <= nev < ncv <= min(ncols, MK_TRLAN_MAX_NCV) and, for a keep that is not 0,
 * nev <= keep < ncv; `which`: 0 = the smallest, 1 = the largest singular values. */
typedef struct {
    mk_params base;
    int32_t nev;              /* eigenpairs (MK_TRSVD: singular triplets) wanted */
    int32_t ncv;              /* MK_TRLAN: basis vectors per cycle; MK_LOBPCG: the block size nb */
    int32_t which;            /* 0 = the smallest ('SA'), 1 = the largest ('LA'); MK_ERR_ARG otherwise */
    int32_t keep;             /* MK_TRLAN: Ritz vectors kept at a restart; 0 = automatic: min(nev + (ncv - nev) / 2, ncv - 1); MK_LOBPCG: must be 0 */
    uint64_t seed;            /* of the hashed start vector (mk_solver_setup with a NULL start); MK_LOBPCG: column j takes seed + j */
} mk_params_eig;

/* The long parameter block of MK_CG's ring of directions (the deferred x update, mk_solver_unapplied below): mk_params followed
 * by a bound on the ring depth m.  Told apart by struct_size = sizeof(mk_params_ring); every solver kind accepts it, only
 * MK_CG reads the tail.  Without it -- and with MK_CG_XDEFER unset -- a set-up takes m = 1 where a vector is at most 256 MiB
 * and otherwise the deepest m <= 32 whose buffers beyond the first two fit an eighth of the device memory that is free: at
 * 512^3 m = 32, 31 GiB beyond the pair.  The bound caps that rule AND an explicit MK_CG_XDEFER (the environment chooses
 * below the caller's bound, never above it).  A placement search (several solver objects alive at once, each probed with a
 * few passes, one kept and set up again) creates its objects with {8, 1}: every probe runs at the same depth and holds 7
 * vectors beyond the pair, and only the kept object's second set-up grows its ring.  The ring grows in mk_solver_setup only
 * and never shrinks while the solver lives.  MK_ERR_ARG unless 0 <= xdefer_cap <= 32 and xdefer_cap_setups >= 0. */
typedef struct {
    mk_params base;
    int32_t xdefer_cap;         /* upper bound on m, 1 .. 32; 0 = none */
    int32_t xdefer_cap_setups;  /* the bound holds for the first k set-ups of the solver object; 0 = for every set-up */
} mk_params_ring;

typedef struct {
    int32_t struct_size;
    int32_t halted;           /* the loop condition of the reference became false */
    int64_t nMatvec;
    int64_t itn;
    int64_t hist_len;         /* entries available through mk_solver_history */
    int32_t converged;
    int32_t definite;         /* cg.py:162 */
    int32_t istop;            /* minres.py:87-98, symmlq.py:99-109 */
    int32_t reserved;
    double residNorm;
    double residNorm0;
    double threshold;
    double Anorm, Acond, Arnorm, ynorm, xnorm;
    double aux[8];            /* MK_CG: [0] the last <p, A p>, [1] the ring depth m of the deferred x update that the last set-up chose
                               * (0: three-kernel passes, 1: x rides in the fused product kernel; mk_params_ring) */
                              /* MK_GMRES: [0] restarts, [1] steps of the last cycle, [2] bytes of the basis */
                              /* MK_IDR: [0] the s in use (after clamping to n), [1] completed cycles, [2] bytes of P, G and U,
                               * [3] breakdown: 0 none, 1 a zero or non-finite pivot M[k,k], 2 a zero or non-finite om */
                              /* MK_PCG: [0] the flexible flag in use, [1] breakdown: 0 none, 1 the curvature test <p, A p> > 0 failed
                               * (`definite` is 0), 2 a <r, M r> that is not positive and finite */
                              /* MK_MSCG: [0] nsigma, [1] breakdown: 0 none, 1 the curvature test <p, A p> > 0 failed (`definite`
                               * is 0), 2 a zero or non-finite term of a shift's zeta recurrence, or a <r, r> that is not positive
                               * and finite, [2] frozen (converged) shifts, [3] bytes of the solver's vectors */
                              /* MK_TRLAN: [0] cycles, [1] the ncv in use, [2] the keep in use, [3] bytes of the basis allocation,
                               * [4] wanted pairs whose estimate met the threshold in the last cycle, [5] breakdown (0 / 1),
                               * [6] Jacobi sweeps of the last cycle's small eigenproblem, [7] milliseconds the device spent in the
                               * last restart's rotation (0 before the first restart) */
                              /* MK_LOBPCG: [0] iterations, [1] the block size nb, [2] active columns of the last iteration,
                               * [3] bytes of the workspace allocation, [4] wanted pairs whose residual met the threshold,
                               * [5] breakdown (0 / 1), [6] Jacobi sweeps of the last small eigenproblem, [7] restarts (small
                               * problems solved again without P, and re-activations of a fully locked block) */
                              /* MK_TRSVD: [0] cycles, [1] the ncv in use, [2] the keep in use, [3] bytes of the two basis allocations,
                               * [4] wanted triplets whose estimate met the threshold in the last cycle, [5] breakdown: 0 none, 1 a
                               * beta, 2 an alpha, 3 a start vector without a positive, finite norm, [6] the reorth in use,
                               * [7] milliseconds the device spent in the last rotation of both bases; `istop` = Jacobi sweeps of
                               * the last cycle's small SVD */
} mk_result;

typedef struct mk_solver mk_solver;

/* MK_GMRES: restarted GMRES(m) with right preconditioning (mk_params.restart, .reorth), every preconditioner setter of the
 * square solvers, single GPU: MK_ERR_UNSUPPORTED for an operator with an exchange plan or a row block, MK_ERR_ARG for a
 * restart outside 1 .. MK_GMRES_MAX_RESTART.  The basis (min(restart, n) + 1 vectors) is allocated at the first set-up;
 * x is complete after every mk_solver_iterate call that observed the halt (the cycle in progress is closed then). */
MK_API int mk_solver_create(const mk_csr *A, const mk_params *params, mk_solver **out);
MK_API int mk_solver_destroy(mk_solver *s);
/* The least-squares solvers (MK_LSQR ... MK_CRAIGMR) need `A.T * u` (lls/lsqr.py:200,264): hand them the
 * transposed matrix (mk_csr_transpose) before mk_solver_setup.  rhs then has nrows(A) entries and x
 * ncols(A) (CRAIG-MR: nrows(A), craigmr.py:112). */
MK_API int mk_solver_set_transpose(mk_solver *s, const mk_csr *At);
/* MK_IDR: IDR(s) in its biorthogonal form with right preconditioning, every preconditioner setter of the square solvers,
 * single GPU: mk_solver_create returns MK_ERR_UNSUPPORTED for an operator with an exchange plan or a row block.  This
 * setter carries its arguments; call it before mk_solver_setup (MK_ERR_STATE afterwards: P, G and U, 3 s vectors, are
 * sized at the first set-up).  `shadow_dim` is s, 1 .. MK_IDR_MAX_S (MK_ERR_ARG otherwise), clamped to n.  `shadow` is
 * NULL -- row k of P is then the hashed field of `seed` + k with entries in [-0.5, 0.5), filled on the device -- or a
 * borrowed device array of shadow_dim * n doubles stored row after row, copied at the first set-up (shadow_dim > n is
 * refused there).  Without the call s = 4 and seed = 1.  MK_ERR_UNSUPPORTED on another solver kind.  A pivot or an om that
 * is zero or not finite halts the run (mk_result.aux[3]); x is the last iterate then, as after every step. */
MK_API int mk_solver_set_idr(mk_solver *s, int32_t shadow_dim, uint64_t seed, const double *shadow);
/* MK_PCG: preconditioned conjugate gradients for symmetric positive definite A and M, z = M r, p = z + beta p, with every
 * preconditioner setter of the square solvers; single GPU (MK_ERR_UNSUPPORTED from mk_solver_create for an operator with an
 * exchange plan or a row block).  mk_params.check_curvature as in MK_CG.  The history holds 2-norms of the recurrence
 * residual of x.  Without a preconditioner the run is MK_CG's bit for bit.  This setter chooses beta: `flexible` 0 (the
 * default without the call) beta = <r,z>' / <r,z>; 1 beta = <z', r' - r> / <r,z>, for a preconditioner that is not the same
 * linear operator at every call (one more inner product per pass).  MK_ERR_ARG unless `flexible` is 0 or 1, MK_ERR_STATE
 * after mk_solver_setup, MK_ERR_UNSUPPORTED on another solver kind.  mk_solver_vector: 0 = r, 1 = p (after a failed
 * curvature test: the direction that failed it; x is then untouched by that pass). */
MK_API int mk_solver_set_pcg(mk_solver *s, int32_t flexible);
/* MK_MSCG: multi-shift conjugate gradients (Frommer and Maass; Jegerlehner, hep-lat/9612014).  Solves (A + sigma_k I) x_k = b
 * for the nsigma shifts of sigma[] in the long parameter block (mk_params_shifts) with ONE product per pass: CG runs on A itself (x_0 = 0, r = p = b)
 * and every shift keeps x_k, p_k and a scalar zeta_k with r_k = zeta_k r, so that its residual norm is |zeta_k| ||r||.  Any
 * finite shift is accepted; the caller answers for A + sigma_k I being positive definite.  It has no function of its own: it
 * enters through the kind and the long parameter block.  mk_solver_create: MK_ERR_ARG for the short block, nsigma outside
 * 1 .. MK_MSCG_MAX_SHIFTS or a shift that is not finite, MK_ERR_UNSUPPORTED for an operator with an exchange plan or a row
 * block (single GPU).  No preconditioner and no initial guess (either destroys the collinearity of the residuals): every
 * preconditioner setter answers MK_ERR_UNSUPPORTED, mk_solver_setup with a guess MK_ERR_ARG.  r, p, q and 2 nsigma vectors
 * are allocated at the first set-up.  threshold = max(abstol, reltol ||b||); after the updates of a pass a shift with
 * |zeta_k| ||r|| <= threshold is frozen: x_k has that pass's update, and from then on neither its vectors nor its scalars
 * are touched.  The loop ends when no shift is active or nMatvec >= matvec_max.  mk_params.check_curvature as in MK_CG: a
 * <p, A p> that is not positive ends the run with nothing updated in that pass (breakdown 1); so does a zero or non-finite
 * term of a zeta recurrence (breakdown 2), every x_k then being its last iterate.
 * mk_solver_x = x_0.  mk_solver_vector: 0 = r, 1 = p (base recurrence), 2 + k = x_k, 2 + nsigma + k = p_k,
 * 2 + 2 nsigma = the per-shift record, len = 3 nsigma: entries 3 k, 3 k + 1, 3 k + 2 hold zeta_k, |zeta_k| ||r|| and the
 * pass at which shift k froze (-1: still active); any other index MK_ERR_ARG.  mk_solver_history = ||r|| of the base
 * recurrence, ||b|| first; mk_solver_history2 = per pass the largest |zeta_k| ||r|| over the shifts that entered the pass
 * active (||b|| first).  mk_result: converged = every shift frozen, residNorm = the largest per-shift residual norm, aux as
 * listed at mk_result. */
/* MK_TRLAN: thick-restart Lanczos (Wu and Simon) for the nev smallest (which = 0) or largest (1) eigenvalues of a symmetric
 * operator and their eigenvectors; the caller answers for the symmetry.  It has no function of its own: it enters through
 * the kind and the long parameter block mk_params_eig.  mk_solver_create: MK_ERR_ARG for the short block, the shifts block or
 * a tail outside the ranges listed at mk_params_eig; MK_ERR_UNSUPPORTED for an operator with an exchange plan or a row
 * block (single GPU).  Every preconditioner setter answers MK_ERR_UNSUPPORTED.
 * mk_solver_setup(s, start_dev, NULL): the start vector, n doubles, borrowed for the call -- for this kind only it may be
 * NULL, which selects the hashed vector mk_cell_field(i, seed) - 1.0 of mk_csr_lanczos.  A guess is MK_ERR_ARG; so are
 * matvec_max < ncv and a start vector whose norm is not positive and finite.  The basis -- ncv + 1 columns and
 * 16 (ceil(keep / 16) - 1) spare ones, each of n rounded up to even plus 2 doubles -- is allocated at the first set-up
 * (MK_ERR_HIP with the sizes if it does not fit).
 * One pass of mk_solver_iterate is one whole cycle: Lanczos steps with full orthogonalisation (classical Gram-Schmidt twice)
 * until the basis is full, without a transfer to the host; then one download of the step scalars, the eigenproblem of the
 * ncv x ncv projected matrix on the host (cyclic Jacobi), one upload of the rotation coefficients and the rotation
 * V[:, :keep] = V S[:, kept] on the device.  est_i = |beta_last S[last, i]| estimates the residual norm of Ritz pair i;
 * threshold = max(abstol, reltol anorm), anorm the largest |Ritz value| seen so far.  The run ends when the nev wanted pairs
 * all have est <= threshold (converged), when a step's beta is not > 2^-26 tmax (breakdown: the basis spans an invariant
 * subspace, every Ritz pair is exact; converged iff it holds at least nev vectors), or when the next cycle's ncv - keep
 * products would exceed matvec_max, which is therefore never exceeded.
 * mk_solver_x = the first eigenvector; mk_solver_vector(i), i < nev: eigenvector i in ascending order of the eigenvalues
 * (after a breakdown with fewer than nev basis vectors only that many are defined); mk_solver_vector(nev) = the record,
 * len = 3 nev: entries 3 i, 3 i + 1, 3 i + 2 hold theta_i, est_i and the cycle (from 1) at which the pair in that place of
 * the wanted order first met the threshold (-1: never); pairs that do not exist hold NaN, NaN, -1.  mk_solver_history = one
 * entry per cycle, the largest estimate among the wanted pairs; mk_solver_history2 = per cycle the milliseconds of its host
 * part (the small eigenproblem, the stop tests and the enqueueing of the rotation: a measurement).  mk_params.window != 0
 * composes the rotation of GmOpCombine launches instead (one output column at a time, keep spare columns; the same bits:
 * the comparison tools/trlan_bench.py makes).  mk_result: itn = Lanczos steps, nMatvec = products,
 * converged and threshold as above, residNorm = the last history entry, residNorm0 = ||start||, aux as listed at
 * mk_result. */
/* MK_LOBPCG: the locally optimal block preconditioned conjugate gradient method (Knyazev 2001) for the nev smallest
 * (which = 0) or largest (1) eigenvalues of a symmetric operator, counted with their multiplicity, and their eigenvectors;
 * the caller answers for the symmetry.  It has no function of its own: it enters through the kind and mk_params_eig, whose
 * `ncv` carries the block size nb.  mk_solver_create: MK_ERR_ARG for the short block, the shifts block or a tail outside the
 * ranges listed at mk_params_eig; MK_ERR_UNSUPPORTED for an operator with an exchange plan or a row block (single GPU).
 * Every preconditioner setter of a square solver works: W_j = precon R_j per active column.  The preconditioner approximates
 * the inverse of A, which steers towards the smallest eigenvalues; the caller keeps it away from which = 1.
 * mk_solver_setup(s, start_dev, NULL): the start block, nb n doubles, column after column, borrowed for the call -- or NULL:
 * column j is the hashed vector mk_cell_field(i, seed + j) - 1.0.  A guess is MK_ERR_ARG; so is matvec_max < nb.  The
 * workspace -- 13 nb columns of n rounded up to even plus 2 doubles (X, W, P and their products twice over, and R), then the
 * partial sums of the Gram kernel -- is one allocation made at the first set-up (MK_ERR_HIP with the sizes if it does not
 * fit).  Set-up forms A X (nb products), solves the first small problem and rotates X.
 * One pass of mk_solver_iterate is one iteration: the host picks the active columns (soft locking: the columns whose residual
 * norm exceeds the threshold; a locked column stays locked), W_j = precon R_j, W <- W - X (X'W) twice, scaled to unit norm,
 * A W (one product per active column), the Gram matrices S'S and S'(A S) of S = [X, W, P] by the tall-skinny Gram kernel
 * (tiles on and above the diagonal), one download of both, the small problem on the host (diagonal scaling, a Cholesky factor
 * with the pivot test v > 2^-26, cyclic Jacobi), one upload of the coefficients, the rotations X <- S C, A X <- (A S) C,
 * P and A P likewise from the W and P rows of C, the residuals R = A X - X diag(theta) with their norms in one kernel, and
 * one download of the nb norms.  A pivot that fails the test drops P and solves the leading problem again (a restart); a
 * second failure ends the run (breakdown: x is the last iterate).  threshold = max(abstol, reltol anorm), anorm the largest
 * |Ritz value| of any small problem so far.  The run ends when the first nev residual norms are all <= threshold
 * (converged), at a breakdown, or when the active products of the next iteration would exceed matvec_max, which is
 * therefore never exceeded.
 * mk_solver_x = the first eigenvector; mk_solver_vector(i), i < nev: eigenvector i in ascending order of the eigenvalues;
 * mk_solver_vector(nev) = the record, len = 3 nev: theta_i, the residual norm ||A x_i - theta_i x_i|| from the loop's own
 * A X, and the iteration (from 0: the start block's own Ritz pairs) at which the pair first met the threshold (-1: never).
 * mk_solver_history = the largest of the first nev residual norms, once for the start block and once per iteration;
 * mk_solver_history2 = the milliseconds of each iteration's host part.  mk_result: itn = iterations, nMatvec = products,
 * residNorm = the last history entry, Anorm = anorm, aux as listed at mk_result.
 * Test hooks of the kind (no function of their own): mk_params.window = 4 or 8 forces the Gram kernel's 4 x 4 or 8 x 8 tile,
 * 1 composes the Gram matrices of GmOpMultiDot launches (the same bits: what tools/lobpcg_bench.py times the kernel
 * against); mk_params.restart = 1 makes the solver a probe of the Gram kernel alone: `ncv` = m, 1 .. 48, columns of n
 * doubles in the start block, set-up forms U'U (the entries on and above the diagonal, mirrored), ends the run, and
 * mk_solver_vector(0) returns the m x m result; aux[7] = the milliseconds of the Gram launches. */
/* MK_TRSVD: thick-restart Golub-Kahan-Lanczos bidiagonalisation (Baglama and Reichel 2005) for the nev largest (which = 1) or
 * smallest (0) singular values of a tall operator A (nrows >= ncols) with their left and right vectors.  It has no function of
 * its own: it enters through the kind and the long parameter block mk_params_eig.  mk_solver_create: MK_ERR_ARG for the short
 * block, the shifts block, a tail outside the ranges listed at mk_params_eig, a mk_params.reorth that is neither 0 nor 1 or a
 * wide operator (nrows < ncols: hand it the transpose and swap the vectors); MK_ERR_UNSUPPORTED for an operator with an
 * exchange plan or a row block (single GPU).  Every preconditioner setter, those of the least-squares solvers included,
 * answers MK_ERR_UNSUPPORTED.  mk_solver_set_transpose hands it A' as it does for the least-squares kinds; mk_solver_setup
 * without it is MK_ERR_STATE.
 * mk_solver_setup(s, start_dev, NULL): the start vector, ncols doubles (the short space), borrowed for the call, or NULL for
 * the hashed vector mk_cell_field(i, seed) - 1.0.  A guess is MK_ERR_ARG.  Both bases are allocated at the first set-up, one
 * allocation each: U of ncv and V of ncv + 1 columns, each with 16 (ceil(keep / 16) - 1) spare ones, a column being the
 * length (nrows for U, ncols for V) rounded up to even plus 2 doubles (MK_ERR_HIP with the sizes if one does not fit).  A
 * start vector without a positive, finite norm, or matvec_max < 2 ncv, halts the run in set-up (MK_OK): no cycle, no
 * triplet, breakdown 3 in the first case.
 * One pass of mk_solver_iterate is one whole cycle, without a transfer to the host: per step u = A v_j, orthogonalised
 * against all of U by classical Gram-Schmidt twice (reorth = 1) or against u_{j-1} alone inside the product kernel
 * (reorth = 0, Simon and Zha's one-sided reorthogonalisation; the first step behind a restart subtracts the arrow
 * sum_i B[i, l+1] u_i by one stream launch per 8 columns), alpha_j = ||u||, u_j = u / alpha_j, w = A' u_j orthogonalised
 * against all of V twice (always), beta_j = ||w||, v_{j+1} = w / beta_j.  Then one download of the step scalars, the SVD of
 * the projected upper triangular matrix B = X diag(s) Y' on the host by a one-sided Jacobi iteration (B'B is never formed),
 * one upload of the rotation coefficients and the rotations of U by X and of V by Y on the device.
 * est_i = |beta_last X[last, i]| is the norm of the whole residual A' u_i - s_i v_i (A v_i = s_i u_i holds to rounding);
 * threshold = max(abstol, reltol anorm), anorm the largest singular value of a projected matrix so far.  The run ends when
 * the nev wanted triplets all have est <= threshold (converged), at a breakdown -- an alpha_j or beta_j that is not
 * > 2^-26 smax, smax the largest alpha or beta accepted so far: the bases span a pair of singular subspaces, every triplet
 * is exact, converged iff they hold at least nev triplets; an alpha breakdown leaves a zero singular value, which is returned
 * as 0 with a zero left vector -- or when the next cycle's 2 (ncv - keep) products would exceed matvec_max, which is
 * therefore never exceeded (products with A and with A' both count).
 * mk_solver_x = the first right vector.  mk_solver_vector(i): i < nev: right vector i (ncols doubles); nev <= i < 2 nev:
 * left vector i - nev (nrows doubles); i = 2 nev: the record, len = 3 nev: entries 3 i, 3 i + 1, 3 i + 2 hold s_i, est_i and
 * the cycle (from 1) at which the triplet in that place of the wanted order first met the threshold (-1: never); the
 * triplets are in descending order of s for either `which`; one that does not exist (a breakdown with fewer than nev steps,
 * a run halted in set-up) holds -1, 0, -1.  mk_solver_history = one entry per cycle, the largest estimate among the wanted
 * triplets; mk_solver_history2 = per cycle the milliseconds of its host part (a measurement).  mk_result: itn = steps,
 * nMatvec = products, converged and threshold as above, residNorm = the last history entry, residNorm0 = ||start||,
 * Anorm = anorm, istop and aux as listed at mk_result. */
/* Several GPUs: mark `A` as THIS rank's block of consecutive rows of a taller m x n operator (its columns are global
 * and unlocalized; no mk_csr_set_exchange).  The least-squares solvers then keep every m-space vector (rhs, u, r;
 * x of CRAIG-MR) sliced like the rows and every n-space vector (v, w, x) whole on every rank: `A * v` needs no
 * exchange, `A.T * u` (lsqr.py:264) is the local transposed block's product summed over the ranks (one all-reduce
 * of n doubles per iteration) and only the m-space inner products are all-reduced.  `At` is the transpose of the
 * local block.  Needs a communicator (mk_comm_init / mk_comm_init_host); without one the flag changes nothing. */
MK_API int mk_csr_set_row_block(mk_csr *A, int on);
/* Diagonal (Jacobi-type) preconditioner: `diag` is a device array with nrows(A) entries holding the diagonal of
 * the operator the reference applies as `precon * r` (cg.py:91-92,137-138; bicgstab.py:96-99,120-123;
 * cgs.py:79-82,88-91; tfqmr.py:77-80; minres.py:162-163,249; symmlq.py:134,228), i.e. what a
 * linop.DiagonalOperator(diag) (linop.py:473-516) multiplies by.  Borrowed: it must stay alive until the solver
 * is destroyed.  NULL removes it.  Call before mk_solver_setup.  MK_ERR_UNSUPPORTED for the lls kinds. */
MK_API int mk_solver_set_precon_diag(mk_solver *s, const double *diag);
/* General preconditioner: any operator the reference would apply as `precon * r` (generic/generic.py:76), evaluated
 * by a HOST callback `fn(user, r_host, y_host)` (n entries each; return 0 on success).  The loop stays on the device: at
 * each preconditioner site the vector is copied to the host, the callback runs, and the inner product that involves
 * its result is formed on the device afterwards.  Not invoked once the loop has halted; in BiCGSTAB / CGS / TFQMR the
 * application that precedes a product happens before that product's loop test, so the callback may run once more
 * than in the reference (its last result is unused; MK_GMRES applies it after the stop test: once per step and once
 * per cycle end; MK_IDR likewise, once per product).  The six square solvers, MK_GMRES, MK_IDR and MK_PCG (once per pass that does not halt, and once at the set-up of a run that does not end there); MK_ERR_UNSUPPORTED for the lls kinds and on partitioned
 * operators.  Replaces a diagonal set earlier.  Call before mk_solver_setup. */
typedef int (*mk_precon_fn)(void *user, const double *r_host, double *y_host);
MK_API int mk_solver_set_precon_callback(mk_solver *s, mk_precon_fn fn, void *user);
/* ... or a DEVICE operator: `precon * r` (generic/generic.py:76) evaluated as a product with a device matrix or
 * composite -- a sparse approximate inverse such as the inverted diagonal blocks of block-Jacobi
 * (pykrylov_amd.tools.block_jacobi) -- at the same sites as the callback, without leaving HBM.  M is borrowed, square,
 * of the solver's (local) size, without an exchange plan (on several GPUs: a rank-local preconditioner).  NULL
 * removes it.  Call before mk_solver_setup. */
MK_API int mk_solver_set_precon_csr(mk_solver *s, const mk_csr *M);
/* Incomplete factorizations of a device matrix A as preconditioners M ~ A (`precon * r` = M^-1 r, generic/generic.py:76),
 * on the pattern of A in CSR column order (stored zeros included; every row must store its diagonal: MK_ERR_ARG otherwise):
 *   mk_ilu0_create: ILU(0), Saad Alg. 10.4 (IKJ form): L unit lower triangular, U upper triangular.  A zero pivot U_ii = 0
 *                   fails with MK_ERR_STATE naming the smallest such row.
 *   mk_ic0_create:  IC(0) of a symmetric matrix (pattern checked; the values of the lower triangle are used): M = L L^T.
 *                   A pivot that is not positive fails with MK_ERR_STATE naming the row.
 * The factor is computed on the device, one launch per level of the forward dependency graph (a host analysis of the
 * pattern groups the rows).  It borrows A's pattern (A may be destroyed meanwhile: it lives on until the factor goes) and
 * owns its values (8 bytes per nonzero) and the row lists of both sweeps.  MK_ERR_UNSUPPORTED for operators that hold no
 * arrays of their own (sums, products, reduced, block, composed, matrix-free: form the matrix first), for operators with an
 * exchange plan, and for nnz >= 2^31.  MK_ERR_ARG for a non-square matrix. */
typedef struct mk_ilu mk_ilu;
MK_API int mk_ilu0_create(const mk_csr *A, mk_ilu **out);
MK_API int mk_ic0_create(const mk_csr *A, mk_ilu **out);
/* Destroying a factor that solvers still hold (mk_solver_set_precon_ilu) is deferred until the last of them goes. */
MK_API int mk_ilu_destroy(mk_ilu *F);
/* out = M^-1 in on device vectors (in == out allowed): forward sweep t_i = r_i - sum_{j<i} L_ij t_j (IC(0): then / l_ii),
 * backward sweep y_i = (t_i - sum_{j>i} U_ij y_j) / U_ii, each row summed left to right in column order.  Rows are
 * solved level by level: one launch per level, or one workgroup for a run of consecutive levels of at most
 * MK_ILU_FUSE_ROWS rows each (environment, read when the factor is created; default 256, 0 = one launch per level). */
MK_API int mk_ilu_apply(const mk_ilu *F, const double *in_dev, double *out_dev);
/* info[k] for k < min(cap, MK_ILU_INFO_LEN): 0 kind (0 ILU(0), 1 IC(0)), 1 rows, 2 nonzeros, 3 / 4 levels of the forward /
 * backward sweep, 5 / 6 launches of the forward / backward sweep, 7 rows of the widest level, 8 device bytes held,
 * 9 fusion threshold in rows, 10 host analysis time (us), 11 factorization time (us). */
#define MK_ILU_INFO_LEN 12
MK_API int mk_ilu_info(const mk_ilu *F, int64_t *info, int32_t cap);
/* The factor to the host: values on A's pattern (nnz doubles; ILU(0): L left of the diagonal, U from it on; IC(0): L
 * left of and on the diagonal, L^T right of it) and the position of every row's diagonal entry (nrows).  Either may be
 * NULL. */
MK_API int mk_ilu_download(const mk_ilu *F, double *values_host, int32_t *diag_host);
/* ... and as the preconditioner of the six square solvers: applied on the device at the sites of the callback (no host
 * round trip), every launch obeying the loop's halt words (nothing changes once the loop has ended).  The solver holds a
 * reference until it is destroyed or the preconditioner is replaced.  Replaces a diagonal, matrix or callback
 * preconditioner; those setters replace it in turn.  NULL removes it.  Single GPU.  Call before mk_solver_setup. */
MK_API int mk_solver_set_precon_ilu(mk_solver *s, const mk_ilu *F);
/* Limited-memory BFGS operators resident in HBM (linop/lbfgs.py): two rings of `npairs` (s, y) columns of n doubles, the
 * scalars ys_k = s_k.y_k, alpha_k and gamma in device memory, partial-sum slots of the object's own, and the Gram entries
 * s_k.s_l, s_k.y_l cached when a pair is stored.  1 <= npairs <= MK_LBFGS_MAX_PAIRS, n >= 1 (MK_ERR_ARG otherwise);
 * `scaling` != 0 scales the initial matrix by gamma = ys / y.y of the newest pair (lbfgs.py:116-120). */
typedef struct mk_lbfgs mk_lbfgs;
#define MK_LBFGS_MAX_PAIRS 64
MK_API int mk_lbfgs_create(int64_t n, int32_t npairs, int32_t scaling, mk_lbfgs **out);
/* Destroying an operator that solvers still hold (mk_solver_set_precon_lbfgs) is deferred until the last of them goes. */
MK_API int mk_lbfgs_destroy(mk_lbfgs *F);
/* lbfgs.py:70-87: the pair (device vectors of n doubles, copied) is rejected (*accepted = 0) when s.y <= threshold (the
 * reference's default is 1e-20), else it overwrites column `insert`, which advances modulo npairs.  s.y, y.y, s.s and the
 * dots of s with every column that stays come from one read of the pair per group of eight dots.  Synchronises. */
MK_API int mk_lbfgs_store(mk_lbfgs *F, const double *s_dev, const double *y_dev, double threshold, int32_t *accepted);
/* lbfgs.py:89-95: forget every pair. */
MK_API int mk_lbfgs_restart(mk_lbfgs *F);
/* out = H in, the inverse approximation by the two-loop recursion (lbfgs.py:97-127) on device vectors (in == out allowed):
 * 2p + 1 launches for p stored pairs (p = 0: a copy, or nothing when in == out); alpha_k and beta are formed on the device
 * in each launch's prologue from the previous launch's partial sums.  Enqueued on the library's stream. */
MK_API int mk_lbfgs_apply(const mk_lbfgs *F, const double *in_dev, double *out_dev);
/* The two halves of the compact forward product (lbfgs.py:188-254) around the small solve the caller makes:
 *   forward_dots:    a[0:p] = (v / gamma) . s_k, a[p:2p] = v . y_k, pairs oldest to newest (2p doubles to the host);
 *   forward_combine: out = v / gamma, then per pair out -= (b_i / gamma) s_k; out -= b_{p+i} y_k (in == out allowed).
 * use_gamma = 0 takes gamma = 1.  Every dot is summed in the order of the library's streaming dot (mk_dot). */
MK_API int mk_lbfgs_forward_dots(const mk_lbfgs *F, const double *in_dev, int32_t use_gamma, double *a_host);
MK_API int mk_lbfgs_forward_combine(const mk_lbfgs *F, const double *in_dev, int32_t use_gamma, const double *coef_host,
                                    double *out_dev);
/* The cached scalars by ring slot (the stored pairs are the slots 0 .. count-1; other entries are NaN): ss[k * npairs + l] =
 * s_k.s_l and sy[k * npairs + l] = s_k.y_l for k stored after l, ss[k * npairs + k] = s_k.s_k, ys[k] = s_k.y_k, yy[k] =
 * y_k.y_k.  Any pointer may be NULL. */
MK_API int mk_lbfgs_gram(const mk_lbfgs *F, double *ss_host, double *sy_host, double *ys_host, double *yy_host);
/* info[k] for k < min(cap, MK_LBFGS_INFO_LEN): 0 n, 1 npairs, 2 scaling, 3 insert, 4 stored pairs, 5 launches of the last
 * apply, 6 applies enqueued, 7 pairs accepted, 8 pairs rejected, 9 device bytes held, 10 column stride (doubles),
 * 11 MK_LBFGS_MAX_PAIRS. */
#define MK_LBFGS_INFO_LEN 12
MK_API int mk_lbfgs_info(const mk_lbfgs *F, int64_t *info, int32_t cap);
/* The rings to the host: slot k to row k of an (npairs, n) array.  Either may be NULL. */
MK_API int mk_lbfgs_download(const mk_lbfgs *F, double *s_host, double *y_host);
/* ... and the inverse operator as the preconditioner of the six square solvers, like mk_solver_set_precon_ilu: applied on
 * the device at the sites of the callback, every launch obeying the loop's halt words; the solver holds a reference until
 * it is destroyed or the preconditioner is replaced; replaces a diagonal, matrix, callback or factorization
 * preconditioner, and those setters replace it in turn; NULL removes it.  Single GPU (MK_ERR_UNSUPPORTED when the
 * solver's operator carries an exchange plan), MK_ERR_ARG on a size mismatch.  Call before mk_solver_setup.  A pair stored
 * between two solves is seen by the next one. */
MK_API int mk_solver_set_precon_lbfgs(mk_solver *s, const mk_lbfgs *F);
/* m = min(steps, nrows) steps of the symmetric Lanczos process on a square, SYMMETRIC device matrix A (the caller vouches
 * for the symmetry), without reorthogonalisation: the tridiagonal T_m = tridiag(beta_j, alpha_j, beta_{j+1}) whose extreme
 * eigenvalues estimate those of A (scale_diag != 0: of D^-1/2 A D^-1/2, D = diag(A), through the diagonally preconditioned
 * recurrence) -- the interval of mk_cheb_create from the matrix instead of the Gershgorin bound.  The recurrence, every
 * operation rounded on its own, in this order:
 *     r2 = start_dev (n doubles, 16-byte aligned), or when NULL r2[i] = u(i, seed) - 1.0 with u the splitmix64 cell field of
 *     mk_csr_poisson3d_varcoef;   y = r2 (scaled: y = dinv * r2, dinv[r] = 1.0 / a_rr);   beta_1 = sqrt(<r2, y>)
 *     step j = 1..m:   s = 1.0 / beta_j;  v = s * y;  t = A v;  j > 1: t = t - (beta_j / beta_{j-1}) * r1;
 *                      alpha_j = <v, t>;  ynew = (-alpha_j / beta_j) * r2 + t;  r1 = r2;  r2 = ynew;
 *                      y = r2 (scaled: dinv * r2);  beta_{j+1} = sqrt(<r2, y>)
 * <v, t> is summed in the order of a dot fused into the product kernel, <r2, y> in that of a stream kernel.  Two launches
 * per step (a storage format that cuts a product into several launches adds its own) plus at most three; all scalars stay
 * on the device until one download at the end, the work vectors are allocated in the call and freed before it returns.
 * The run stops on the device after step j when beta_{j+1} is not > 2^-26 * max_{i<=j}(|alpha_i| + [i>1] * beta_i)
 * (breakdown: every Ritz value is then an eigenvalue to sqrt(eps)), or when alpha_j or beta_{j+1} is not finite.
 * Output, with `done` the steps completed: alpha_host[0 .. done) = alpha_1.., beta_host[0 .. done] = beta_1.. (beta_1 is
 * the norm of the start vector and no entry of T); the arrays hold min(steps, nrows) and min(steps, nrows) + 1 doubles.
 * info[k] for k < min(cap, MK_LANCZOS_INFO_LEN): 0 steps completed, 1 launches, 2 device bytes used, 3 elapsed time (us),
 * 4 whether a scalar was not finite.
 * MK_ERR_ARG for a non-square matrix, steps < 1, a matrix without rows, beta_1 zero or not finite, an alpha or beta that is
 * not finite (the message gives the step) and -- with scale_diag -- a row whose diagonal entry is missing, zero or negative
 * (the message names the smallest such row).  MK_ERR_UNSUPPORTED for operators that hold no arrays of their own and for
 * operators with an exchange plan. */
#define MK_LANCZOS_INFO_LEN 5
MK_API int mk_csr_lanczos(const mk_csr *A, int32_t steps, int32_t scale_diag, uint64_t seed, const double *start_dev,
                          double *alpha_host, double *beta_host, int64_t *info, int32_t cap);
/* Chebyshev polynomial preconditioner z = p_k(A) r of a square, SYMMETRIC device matrix A (the caller vouches for the
 * symmetry): the Chebyshev iteration for A z = r from z = 0 on an interval [lmin, lmax], 0 < lmin < lmax, that should hold
 * A's spectrum (Saad, Iterative Methods, Alg. 12.1); with scale_diag != 0 the iteration for D^-1 A z = D^-1 r, D = diag(A).
 * 1 <= degree <= MK_CHEB_MAX_DEGREE.  lmax <= 0 on input takes the Gershgorin bound max_r sum_j |a_rj| (scaled: / |a_rr|),
 * computed on the device, each row added left to right in stored order; lmin <= 0 takes lmax / 30 (the convention of hypre
 * and Ifpack2 where no lower estimate is given).  The coefficients depend on lmin, lmax and degree only and are computed
 * once on the host, one rounding per operation:
 *     theta = 0.5*(lmax+lmin);  delta = 0.5*(lmax-lmin);  sigma = theta/delta;  c0 = 1.0/theta;  rho_0 = 1.0/sigma
 *     j = 1..k:  rho_j = 1.0/(2.0*sigma - rho_{j-1});  c1_j = rho_j*rho_{j-1};  c2_j = (2.0*rho_j)/delta
 * The object borrows A (A may be destroyed meanwhile: it lives on until the object goes) and owns three vectors of nrows
 * doubles, and 1 / a_rr when scaled.  MK_ERR_ARG for a non-square matrix, a degree out of range, non-finite bounds, an
 * interval without 0 < lmin < lmax, and -- with scale_diag -- a row that stores no diagonal entry or a zero one (the message
 * names the smallest such row).  MK_ERR_UNSUPPORTED for operators that hold no arrays of their own and for operators with an
 * exchange plan. */
typedef struct mk_cheb mk_cheb;
#define MK_CHEB_MAX_DEGREE 64
MK_API int mk_cheb_create(const mk_csr *A, int32_t degree, double lmin, double lmax, int32_t scale_diag, mk_cheb **out);
/* Destroying an object that solvers still hold (mk_solver_set_precon_cheb) is deferred until the last of them goes. */
MK_API int mk_cheb_destroy(mk_cheb *F);
/* out = p_k(A) in on device vectors (in == out allowed; out of place, `in` is not modified): one stream launch
 *     res = in (scaled: dinv * in);  d_0 = res * c0;  out = d_0
 * then per step j = 1..k one product of A on d_{j-1}, in the storage format A has, whose row epilogue does, in this order,
 *     s = row sum (scaled: s = dinv_r * s);  rv = res_r - s;  d_j = c1_j * d_{j-1,r} + c2_j * rv;  out_r = out_r + d_j;  res_r = rv
 * with one rounding per operation.  Enqueued on the library's stream. */
MK_API int mk_cheb_apply(const mk_cheb *F, const double *in_dev, double *out_dev);
/* info[k] for k < min(cap, MK_CHEB_INFO_LEN): 0 rows, 1 degree, 2 scaled, 3 launches per apply (1 + degree; a storage format
 * that cuts a product into several launches adds its own), 4 device bytes held, 5 set-up time (us), 6 / 7 whether lmin / lmax
 * is the default. */
#define MK_CHEB_INFO_LEN 8
MK_API int mk_cheb_info(const mk_cheb *F, int64_t *info, int32_t cap);
/* 3 + 2 * degree doubles to the host: lmin and lmax as used, c0, then c1_1, c2_1, ..., c1_k, c2_k. */
MK_API int mk_cheb_coefficients(const mk_cheb *F, double *host);
/* ... and as the preconditioner of the six square solvers, like mk_solver_set_precon_ilu: applied on the device at the
 * sites of the callback, every launch obeying the loop's halt words; the solver holds a reference until it is destroyed or
 * the preconditioner is replaced; NULL removes it.  Single GPU, MK_ERR_ARG on a size mismatch.  Call before
 * mk_solver_setup. */
MK_API int mk_solver_set_precon_cheb(mk_solver *s, const mk_cheb *F);
/* The third long parameter block: mk_params_eig followed by a scaled Chebyshev filter rho(A) (Zhou and Saad), the spectral
 * transformation of MK_TRLAN.  Told apart by struct_size = sizeof(mk_params_filter); every other kind answers
 * MK_ERR_UNSUPPORTED to it.  It adds no function: the solver creates the filter at mk_solver_create and owns it.
 * A must be a square SYMMETRIC device matrix with CSR arrays of its own, single GPU (the caller vouches for the symmetry).
 * [a, b] is the UNWANTED interval, a0 a reference point strictly outside it on the wanted side (a0 < a: which = 0, a0 > b:
 * which = 1), and
 *     rho(t) = T_d((t - c)/e) / T_d((a0 - c)/e),   e = 0.5*(b - a),  c = 0.5*(b + a),   d = degree, 1 .. MK_FILTER_MAX_DEGREE.
 * The coefficients are computed once on the host, one rounding per operation, in this order:
 *     sigma_1 = e/(a0 - c);  tau = 2.0/sigma_1;  p_1 = sigma_1/e;  q_1 = 0
 *     j = 2..d:  sigma_j = 1.0/(tau - sigma_{j-1});  p_j = (2.0*sigma_j)/e;  q_j = sigma_{j-1}*sigma_j
 * An end of the interval given as NaN is taken from the Gershgorin interval of the matrix, computed on the device:
 * [min_r (a_rr - off_r), max_r (a_rr + off_r)], off_r = sum_{j != r} |a_rj|, each row added left to right in stored order from
 * +0.0 (stored entries on the diagonal add up to a_rr), the minimum and the maximum taken through an order-preserving integer
 * key.  The filter owns min(degree - 1, 2) vectors of nrows doubles.  out = rho(A) in is `degree` products of A, in the
 * storage format A has; the row epilogue of step j = 1..d on y_{j-1} (y_0 = in) does
 *     t = s - c*y_{j-1,r};  y_j = p_j*t;  y_j = y_j - q_j*y_{j-2,r}        (s the row sum; step 1 has no y_{-1} term)
 * with one rounding per operation.  mk_solver_create: MK_ERR_ARG for a non-square matrix, a degree out of range, an infinite
 * end, a >= b, an a0 that is not finite or lies inside [a, b], coefficients that are not finite, and a `which` that does not
 * name the side a0 lies at; MK_ERR_UNSUPPORTED for operators that hold no arrays of their own, with an exchange plan or a
 * row block.
 * mk_solver_vector(s, nev + 1) = the filter's table, 5 + 2 degree + 8 doubles: a, b and a0 as used, c, e, p_1, q_1, ..., p_d,
 * q_d, then rows, degree, the wanted side (0 smallest, 1 largest), launches per apply, device bytes held, set-up time (us),
 * whether a / b is the Gershgorin end.
 * The filtered cycle, per cycle:
 *   - the product of every Lanczos step is the filter (d launches); orthogonalisation, the small eigenproblem and the
 *     rotation are unchanged; B's Ritz values are taken in descending order whatever `which` says (rho is positive and
 *     monotone on the wanted side);
 *   - B's estimates |beta S[last, i]| <= max(abstol, reltol anorm_B) only open a gate.  Once the gate has been met, and in
 *     the last cycle the budget allows, the restart rotation is followed by the verification on A: for each of the first nev
 *     kept vectors x one product of A, theta = <x, A x>, and ||A x - theta x||; the run has converged when every such norm is
 *     at most max(abstol, reltol anorm_A), anorm_A = max(|a|, |b|, |a0|).  Otherwise it goes on from the restart;
 *   - nMatvec counts every product of A (filter steps and verification); a cycle starts only if its (ncv - l) d + nev products
 *     fit into matvec_max (l = 0 in the first cycle, keep afterwards; mk_solver_setup answers MK_ERR_ARG if the first does not).
 * The record (mk_solver_vector(nev)) holds theta_A ascending, the true A-residual norms (NaN where none was computed) and the
 * cycle at which B's estimate first met the gate; mk_solver_vector(i) the verified vectors in that order; mk_solver_history one
 * entry per cycle, the largest A-residual where the cycle was verified and B's largest estimate otherwise.  mk_result:
 * residNorm the last history entry, threshold and Anorm those of A, aux[4] the pairs whose A-residual met the threshold.
 * The probe (mk_params.restart = 1 with this block): no Lanczos run; mk_solver_setup(s, in_dev, NULL) enqueues
 * out = rho(A) in, `in` unchanged, and ends the run; mk_solver_x = out (owned by the solver, overwritten by the next
 * set-up); `which` is not compared with the side.  It is how tools.ChebyshevFilter applies the filter to a vector. */
#define MK_FILTER_MAX_DEGREE 128
typedef struct {
    mk_params_eig eig;
    int32_t degree;           /* 1 .. MK_FILTER_MAX_DEGREE */
    int32_t filter_reserved;
    double a, b;              /* the unwanted interval; NaN: the Gershgorin end */
    double a0;                /* the reference point */
} mk_params_filter;
/* FSAI (factorized sparse approximate inverse, Kolotilina and Yeremin) of a square, symmetric positive definite device
 * matrix A ~ L L': a sparse lower-triangular G ~ L^-1 on a fixed pattern, computed on the device; the preconditioner is
 * M^-1 = G' G.  A owns CSR arrays with sorted rows and no duplicates (as for mk_ilu0_create); it is read during the call only
 * and not borrowed afterwards.
 * The pattern: pat_indptr_host / pat_indices_host (n + 1 and pat_indptr_host[n] host ints), or both NULL for the stored
 * lower triangle of A, diagonal included (extracted on the device).  A given pattern is lower triangular, every row sorted
 * without duplicates and ending with its diagonal entry; no row has more than MK_FSAI_MAX_ROW entries.
 * Row i with pattern columns P[0] < ... < P[m-1] = i, one rounding per operation, every sum sequential in the order written
 * (so the result does not depend on how rows and entries are assigned to lanes):
 *     gather    S[a][b] = A[P[a], P[b]] for b <= a, read from the lower part of row P[a] of A; a position A does not store
 *               counts as 0.0
 *     Cholesky  s = S[a][b]; for k = 0 .. b-1: s = s - L[a][k] * L[b][k];  L[a][a] = sqrt(s);  L[a][b] = s / L[b][b]
 *     solve     y[m-1] = 1.0 / L[m-1][m-1];  for a = m-1 .. 0: s = y[a] (0.0 for a < m-1);
 *               for k = m-1 .. a+1: s = s - L[k][a] * y[k];  y[a] = s / L[a][a]
 *     scaling   g = y / sqrt(y[m-1])            (then diag(G A G') = 1)
 * G and G' (mk_csr_transpose of G) are kept as device matrices and get the storage formats their patterns earn.
 * MK_ERR_ARG for a non-square matrix, a row of A without a stored diagonal entry (pattern from A), a pattern that is not as
 * described (the message names the first bad row), a pattern row that is longer than MK_FSAI_MAX_ROW (the message names the
 * row and its length) and a diagonal s of a Cholesky factor that is not > 0 or not finite (the message names the smallest
 * such row).  MK_ERR_UNSUPPORTED for operators that hold no arrays of their own and for operators with an exchange plan. */
typedef struct mk_fsai mk_fsai;
#define MK_FSAI_MAX_ROW 32
MK_API int mk_fsai_create(const mk_csr *A, const int32_t *pat_indptr_host, const int32_t *pat_indices_host, mk_fsai **out);
/* Destroying an object that solvers still hold (mk_solver_set_precon_fsai) is deferred until the last of them goes. */
MK_API int mk_fsai_destroy(mk_fsai *F);
/* out = G' (G in) on device vectors (in == out allowed; out of place, `in` is not modified): two products, tmp = G in and
 * out = G' tmp, each a row sum from left to right in whatever storage format the matrix has.  Enqueued on the library's
 * stream. */
MK_API int mk_fsai_apply(const mk_fsai *F, const double *in_dev, double *out_dev);
/* info[k] for k < min(cap, MK_FSAI_INFO_LEN): 0 rows, 1 nonzeros of G, 2 longest row of G, 3 launches per apply (2; a storage
 * format that cuts a product into several launches adds its own), 4 device bytes held (the CSR arrays of G and G' and one
 * vector; not what their storage formats add), 5 / 6 storage format of G / of G' (built by this call if need be), 7 set-up
 * time (us). */
#define MK_FSAI_INFO_LEN 8
MK_API int mk_fsai_info(const mk_fsai *F, int64_t *info, int32_t cap);
/* G as CSR arrays to the host: rows + 1 ints, nnz ints, nnz doubles (info 0 and 1); a NULL array is skipped. */
MK_API int mk_fsai_download(const mk_fsai *F, int32_t *indptr_host, int32_t *indices_host, double *values_host);
/* The two matrices the object owns, borrowed (for mk_csr_set_format / mk_csr_format_info; never destroy them); either
 * pointer may be NULL. */
MK_API int mk_fsai_factors(const mk_fsai *F, mk_csr **G, mk_csr **Gt);
/* ... and as the preconditioner of the square solvers, exactly like mk_solver_set_precon_cheb. */
MK_API int mk_solver_set_precon_fsai(mk_solver *s, const mk_fsai *F);
/* Smoothed-aggregation algebraic multigrid (Vanek, Mandel, Brezina) of a square, SYMMETRIC device matrix A with a positive
 * stored diagonal (the caller vouches for the symmetry): the hierarchy is set up on the device, an apply is one V(1,1)-cycle.
 * A owns CSR arrays with sorted rows and no duplicates; the object borrows it (A may be destroyed meanwhile: it lives on until
 * the object goes).  Every operation is rounded on its own and every sum is sequential in the order written, formed by one
 * lane, so the hierarchy does not depend on grids, on atomics or on `expand_cap`.  Per level, A_0 = A:
 *   1 diagonal, bound   d_i = the first stored a_ii;  dinv_i = 1.0 / d_i;  lmax = max_i (sum_j |a_ij|) / |a_ii|, the row added
 *                       left to right in stored order from 0.0 -- the Gershgorin bound of mk_cheb_create(scale_diag = 1).  The
 *                       level's smoother S is mk_cheb_create(A_l, degree, lmax / ratio, lmax, 1).
 *   2 strength          a stored entry v = a_ij, j != i, v != 0 is strong iff  v * v > ((theta * theta) * d_i) * d_j.
 *   3 MIS(2) roots      (Bell, Dalton, Olson 2012)  key_i = state << 62 | h30(i) << 32 | i, state 2 in / 1 undecided / 0 out,
 *                       every node undecided at first.  h30(i) = z >> 34 with z the splitmix64 word of the cell field of
 *                       mk_csr_poisson3d_varcoef for cell i:  z = (i + 1) * 0x9E3779B97F4A7C15 + seed (mod 2^64);
 *                       z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z = z ^ z >> 31.
 *                       Only i and `seed` feed it: the same on every level.  A round: m1_i = max(key_i, key_j over the strong
 *                       entries of row i), m2_i = the same of m1 (each from one buffer into another); then an undecided node
 *                       with m2_i == key_i goes in, one whose m2_i has state 2 goes out.  Rounds repeat until a device
 *                       counter of undecided nodes, read by the host once per round, is zero.
 *   4 aggregates        the roots (state 2) are numbered in index order by an exclusive scan (on the device).  Pass 1: a root
 *                       takes its number; another node takes the number of the root among its strong entries with the largest
 *                       |a_ij|, the first in stored order on ties; else -1.  Pass 2, reading pass 1's buffer: a node left at
 *                       -1 takes pass 1's value of the strong entry with the largest |a_ij| among those pass 1 assigned, the
 *                       first on ties.  A node without strong entries is a root and a singleton.
 *   5 prolongator       P = T - (omega / lmax) D^-1 (A T), T[i, agg(i)] = 1.0.  Row i is the list (agg(i), 1.0), then
 *                       (agg(j), (-((omega / lmax) * dinv_i)) * a_ij) over the stored entries of row i in order; the list is
 *                       stable-sorted by column and duplicates are summed in list order from 0.0 (the rule of
 *                       mk_csr_from_coo).  R = mk_csr_transpose(P).
 *   6 Galerkin product  A_{l+1} = R (A_l P), two products C = X Y: row i of C is the list (j, x_ik * y_kj) over the entries of
 *                       row i of X in order and within each over the entries of row k of Y in order, compressed as above.  The
 *                       lists are expanded in chunks of whole rows of at most `expand_cap` entries (a longer row alone;
 *                       0 = 2^26 entries, 24 bytes each while a chunk is compressed; at most 2^31 - 1).
 *   7 stopping          no further level when n_l <= coarse_max, when the hierarchy has max_levels levels, or when a level
 *                       has as many aggregates as rows.
 *   8 coarsest level    n <= coarse_max: downloaded, factored on the host by the Cholesky recurrence of mk_fsai_create over
 *                       the dense lower triangle (s = a[a][b]; k = 0 .. b-1: s = s - L[a][k] * L[b][k]; L[a][a] = sqrt(s),
 *                       L[a][b] = s / L[b][b]), then column c of the inverse:  a = 0 .. n-1: s = (a == c ? 1.0 : 0.0);
 *                       k = 0 .. a-1: s = s - L[a][k] * y[k]; y[a] = s / L[a][a];  a = n-1 .. 0: s = y[a]; k = n-1 .. a+1:
 *                       s = s - L[k][a] * x[k]; x[a] = s / L[a][a];  Ainv[a][c] = x[a].  Uploaded as a dense matrix.  A pivot
 *                       that is not positive and finite, or a larger last level: the level is solved by its smoother alone.
 * The cycle on level l, with S the level's mk_cheb_apply:  x = S(b);  r = b - A x;  b_{l+1} = R r;  e = cycle(l + 1, b_{l+1});
 * x = x + P e;  r = b - A x;  x = x + S(r).  On the coarsest level x = Ainv b, each row summed left to right from 0.0 (or
 * x = S(b)).  Residual and correction are row epilogues of the products of A_l and P in whatever storage format the matrices
 * have; R r is a plain product.
 * 1 <= degree <= MK_CHEB_MAX_DEGREE, ratio > 1, omega > 0, theta >= 0, 1 <= coarse_max <= MK_AMG_MAX_COARSE,
 * 1 <= max_levels <= MK_AMG_MAX_LEVELS, 0 <= expand_cap < 2^31: MK_ERR_ARG otherwise, for a non-square matrix and for a row,
 * on any level, whose diagonal entry is missing, zero, negative or not finite (the message names the smallest such row and the
 * level).  MK_ERR_UNSUPPORTED for operators that hold no arrays of their own and for operators with an exchange plan. */
typedef struct mk_amg mk_amg;
#define MK_AMG_MAX_LEVELS 16
#define MK_AMG_MAX_COARSE 1024
MK_API int mk_amg_create(const mk_csr *A, double theta, int32_t degree, double ratio, double omega, int32_t coarse_max,
                         int32_t max_levels, uint64_t seed, int64_t expand_cap, mk_amg **out);
/* Destroying an object that solvers still hold (mk_solver_set_precon_amg) is deferred until the last of them goes. */
MK_API int mk_amg_destroy(mk_amg *F);
/* out = one V(1,1)-cycle on in, device vectors (in == out allowed; out of place, `in` is not modified).  Enqueued on the
 * library's stream. */
MK_API int mk_amg_apply(const mk_amg *F, const double *in_dev, double *out_dev);
/* info[k] for k < min(cap, MK_AMG_INFO_LEN).  level = -1, the totals: 0 levels, 1 device bytes held (the levels' CSR arrays, P, R,
 * vectors, smoothers, the coarse inverse; not what storage formats add), 2 set-up time (us), 3 launches per apply ((7 + 2 degree)
 * per level but the last, 1 or 1 + degree on the last; a storage format that cuts a product into several launches adds its own),
 * 4 the coarsest level is solved by 1 the dense inverse, 0 its smoother alone, 5 operator complexity x 1000 (sum of nnz(A_l) /
 * nnz(A_0), rounded), 6 grid complexity x 1000, 7 sum of nnz(A_l), 8 sum of the levels' rows, 9 why there is no inverse: 0 there is
 * one, 1 the last level has more than coarse_max rows, 2 a pivot was not positive.
 * level >= 0: 0 rows, 1 nnz of A_l, 2 nnz of P (0 on the last level), 3 aggregates, 4 MIS(2) rounds, 5 / 6 entries of the expanded
 * lists of A P / of R (A P), 7 / 8 chunks they took, 9 chunks of P's list. */
#define MK_AMG_INFO_LEN 10
MK_API int mk_amg_info(const mk_amg *F, int32_t level, int64_t *info, int32_t cap);
/* A matrix of a level, borrowed (for mk_csr_download / mk_csr_set_format / mk_csr_format_info; never destroy it): which = 0 A_l,
 * 1 P, 2 R (MK_ERR_ARG on the last level, which has neither). */
MK_API int mk_amg_level(const mk_amg *F, int32_t level, int32_t which, mk_csr **borrowed);
/* agg (rows of the level ints; not on the last level) and lmax of a level to the host; either may be NULL. */
MK_API int mk_amg_download(const mk_amg *F, int32_t level, int32_t *agg_host, double *lmax_host);
/* The coarse inverse, row major, n_last * n_last doubles.  MK_ERR_STATE when the coarsest level is solved by its smoother. */
MK_API int mk_amg_coarse(const mk_amg *F, double *inverse_host);
/* ... and as the preconditioner of the square solvers, exactly like mk_solver_set_precon_cheb. */
MK_API int mk_solver_set_precon_amg(mk_solver *s, const mk_amg *F);
/* The least-squares kinds take two preconditioners, applied by the reference as `u = M(Mu)` in the m-space and
 * `v = N(Nv)` in the n-space of the Golub-Kahan process (lls/lsqr.py:189-190,201-202,253-254,265-266 and the same
 * lines of lsmr.py, craig.py, craigmr.py).  Each side holds ONE preconditioner of any of the kinds the square solvers
 * take -- a diagonal, a host callback, a device matrix or composite, an incomplete factorization, an inverse L-BFGS
 * operator, a Chebyshev polynomial preconditioner, an FSAI preconditioner, an AMG preconditioner -- and every setter below replaces what its side held (releasing the reference it kept on a matrix or object)
 * without touching the other side.  MK_ERR_UNSUPPORTED for the six square solvers.  Call before mk_solver_setup.
 *
 * Diagonals: device arrays with the diagonals of M (nrows(A) entries) and N (ncols(A) entries), multiplied inside the
 * kernels; borrowed until the solver is destroyed.  A NULL side loses a diagonal set earlier and keeps anything else. */
MK_API int mk_solver_set_lls_precon(mk_solver *s, const double *diag_m, const double *diag_n);
/* M and / or N as HOST callbacks `fn(user, in_host, out_host)` -- any callable the reference would apply as
 * `u = M(Mu)` (nrows(A) entries) or `v = N(Nv)` (ncols(A) entries); a NULL function removes a callback set earlier and
 * leaves anything else on that side.  The loop stays on the device: the vector is copied to the host right after the kernel
 * that formed it, the callback's result replaces u / v and <u, Mu> / <v, Nv> are re-formed on the device.  Not invoked once
 * the loop has halted, nor for N when beta = 0 (lsqr.py:258).  Single GPU. */
MK_API int mk_solver_set_lls_precon_callback(mk_solver *s, mk_precon_fn fn_m, void *user_m, mk_precon_fn fn_n, void *user_n);
/* M or N (`side`) as a DEVICE preconditioner, applied at the sites of the callback without leaving HBM and with its bits:
 * u / v is replaced right after the kernel that formed Mu / Nv and <u, Mu> / <v, Nv> is re-formed in the same order.  Every
 * launch obeys the loop's halt words (nothing changes once the loop has ended), and N is not applied when beta = 0
 * (lsqr.py:258) -- both decided on the device, without a host read.
 *   _csr:   a device matrix or composite (e.g. pykrylov_amd.tools.block_jacobi), square, of that side's size (nrows(A) for
 *           M, ncols(A) for N), without an exchange plan; counted among the matrix's dependents while the side holds it.
 *   _ilu:   an incomplete factorization (mk_ilu0_create / mk_ic0_create) of that side's size.
 *   _bfgs:  an inverse L-BFGS operator (mk_lbfgs) of that side's size; a pair stored between two solves is seen by the
 *           next one.  (Spelt _bfgs on purpose: the names that contain "lbfgs" are the operator's own entry points and the
 *           square solvers' mk_solver_set_precon_lbfgs, a closed set that tests/test_lbfgs_cpu.py pins name by name.)
 *   _cheb:  a Chebyshev polynomial preconditioner (mk_cheb_create) of a symmetric matrix of that side's size.
 *   _fsai:  an FSAI preconditioner (mk_fsai_create) of a symmetric positive definite matrix of that side's size.
 *   _amg:   an AMG preconditioner (mk_amg_create) of a symmetric matrix of that side's size.
 * The solver holds a factor or operator until it is destroyed or the side is given something else: destroying the object
 * meanwhile is deferred.  NULL removes what the side holds.  MK_ERR_ARG on a size mismatch or a non-square matrix.
 * Single GPU: with row blocks over several GPUs (mk_csr_set_row_block) only diagonals are supported, mk_solver_setup fails
 * with MK_ERR_UNSUPPORTED otherwise. */
enum { MK_LLS_SIDE_M = 0, MK_LLS_SIDE_N = 1 };
MK_API int mk_solver_set_lls_precon_csr(mk_solver *s, int side, const mk_csr *P);
MK_API int mk_solver_set_lls_precon_ilu(mk_solver *s, int side, const mk_ilu *F);
MK_API int mk_solver_set_lls_precon_bfgs(mk_solver *s, int side, const mk_lbfgs *F);
MK_API int mk_solver_set_lls_precon_cheb(mk_solver *s, int side, const mk_cheb *F);
MK_API int mk_solver_set_lls_precon_fsai(mk_solver *s, int side, const mk_fsai *F);
MK_API int mk_solver_set_lls_precon_amg(mk_solver *s, int side, const mk_amg *F);
/* Everything before the `while` loop of the reference's solve().  rhs_dev has n_local
 * entries; guess_dev may be NULL (x0 = 0).  Neither is modified. */
MK_API int mk_solver_setup(mk_solver *s, const double *rhs_dev, const double *guess_dev);
/* Run at most max_iters further passes of the loop body entirely on the device (no
 * host round trip per iteration); stops early when the reference's loop condition
 * fails.  iters_done may be NULL. */
MK_API int mk_solver_iterate(mk_solver *s, int64_t max_iters, int64_t *iters_done);
/* Everything after the loop (e.g. SYMMLQ's CG-point transfer) + result scalars. */
MK_API int mk_solver_finish(mk_solver *s, mk_result *res);
MK_API int mk_solver_x(const mk_solver *s, const double **x_dev);
MK_API int mk_solver_history(const mk_solver *s, double *hist_host, int64_t cap);
/* 1 when the solver runs FUSED passes: CG (cg.py:113-158) on a single-device matrix in storage format 9 applies a pass's
 * `x += alpha p ; p = beta p - r` (cg.py:130,150-151) inside the NEXT pass's product kernel, which loads the rows of p, r
 * and x once for both (one sweep over p less per iteration; every bit of x, p, r and of the history unchanged).  The
 * product kernel then moves 48 bytes per row besides the matrix data (p, r, x in; p, x, A p out) instead of 16.
 * mk_solver_x / mk_solver_vector always hand out the up-to-date iterate (formed into scratch vectors between passes).
 * Environment MK_CG_FUSE=0 turns it off.  Valid after mk_solver_setup. */
MK_API int mk_solver_fused(const mk_solver *s, int32_t *fused);
/* Fused CG passes with a DEFERRED x update (environment MK_CG_XDEFER = m, 1 ... 32; default 1 where a vector is at most
 * 256 MiB, else the deepest m <= 32 that fits an eighth of the free device memory, see mk_params_ring): x is an accumulator that the loop never reads, so the product kernel leaves it alone (33 bytes per row
 * besides the matrix data: p, r in; p, A p out), the directions stay in a ring of m + 1 buffers and one sweep applies m of
 * them to x -- each `x += alpha p` rounded on its own, in order: every bit unchanged.  mk_solver_iterate applies whatever its
 * passes left before it returns, so this count -- completed passes whose direction has not reached x yet -- is 0 after every
 * call (with m = 1 it is 1 between passes: that update rides in the next product kernel).  Valid after mk_solver_setup. */
MK_API int mk_solver_unapplied(const mk_solver *s, int64_t *count);
/* Second per-iteration channel, same length as the history (MINRES: truncated direct-error
 * estimate / energy norm, `dir_errors_window` of minres.py:307-308; NaN while itn <= window). */
MK_API int mk_solver_history2(const mk_solver *s, double *hist_host, int64_t cap);
/* Other device vectors of the loop by solver-specific index (CG: 0 = r, 1 = p, the
 * direction stored as `infiniteDescent`, cg.py:122).  len may be NULL. */
MK_API int mk_solver_vector(const mk_solver *s, int index, const double **v_dev, int64_t *len);
/* Device time of the last mk_solver_iterate call (HIP events on the solver's stream)
 * and the accumulated time/launch count of its SpMV kernel. */
MK_API int mk_solver_timing(const mk_solver *s, double *iterate_ms, double *spmv_ms, int64_t *spmv_launches);
/* Average duration of the solver's fused SpMV kernel: `launches` back-to-back launches of exactly the
 * kernel a loop pass uses, bracketed by ONE pair of HIP events on the solver's stream (a pair around
 * each single launch would add ~3-6 us of marker overhead to a ~20 us kernel).  Destroys the product
 * vector of the current pass: call it after the timed iterations. */
MK_API int mk_solver_time_spmv(mk_solver *s, int64_t launches, double *avg_us);
/* The same for a chosen product of the pass: which = 0 the first (every solver; = mk_solver_time_spmv), 1 the second --
 * BiCGSTAB's `A z` with its three fused dots (bicgstab.py:125), CGS's `A z` with `r -= alpha A z` (cgs.py:96-100),
 * TFQMR's second `A z` (tfqmr.py:145-147), the least-squares solvers' `A.T * u` with the fused v update (lsqr.py:264).
 * Launched without the loop gate.  MK_ERR_ARG if the solver has no such product. */
MK_API int mk_solver_time_product(mk_solver *s, int which, int64_t launches, double *avg_us);
/* One-shot convenience: setup + iterate(until halted) + finish. */
MK_API int mk_solver_solve(mk_solver *s, const double *rhs_dev, const double *guess_dev, mk_result *res);

#ifdef __cplusplus
}
#endif
#endif /* MIKRYLOV_H */
