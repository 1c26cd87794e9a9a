// mk_core.hip -- context, memory, CSR container, standalone SpMV / BLAS-1 entry points and
// the on-device matrix generators of libmikrylov (C ABI in include/mikrylov.h).
#include <stdarg.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <thread>

#include "mk_solver.h"

// ======================================================================================
// context
// ======================================================================================
MkContext &mk_ctx() {
    static MkContext ctx;
    return ctx;
}

int mk_fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    mk_ctx().last_error = buf;
    return code;
}

static int *g_halt0 = nullptr;   // two zero ints: "never halted" flags for standalone kernels

static_assert(mk_switch_table[MK_SW_GRID_STREAM].hi == MK_MAXP && mk_switch_table[MK_SW_GRID_SPMV].hi == MK_MAXP, "grid caps <= MK_MAXP");
int mk_cap_stream() { return (int)mk_switch_int<MK_SW_GRID_STREAM>(); }
int mk_cap_spmv() { return (int)mk_switch_int<MK_SW_GRID_SPMV>(); }

extern "C" int mk_version(void) { return MK_VERSION; }

extern "C" const char *mk_last_error(void) { return mk_ctx().last_error.c_str(); }

extern "C" int mk_init(int device) {
    MkContext &c = mk_ctx();
    if (c.ready && c.device == device) return MK_OK;
    if (c.ready) return mk_fail(MK_ERR_STATE, "mk_init: already bound to device %d", c.device);
    int count = 0;
    MK_HIP(hipGetDeviceCount(&count));
    if (count <= 0) return mk_fail(MK_ERR_HIP, "mk_init: no HIP device visible");
    MK_ARG(device >= 0 && device < count);
    MK_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    MK_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_init: device is %s; this library is built for gfx950 only",
                       prop.gcnArchName);
    c.num_cu = prop.multiProcessorCount;
    MK_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    MK_HIP(hipHostMalloc((void **)&c.h_scratch, sizeof(double) * MK_MAXP * MK_NDOT, hipHostMallocDefault));
    MK_HIP(hipMalloc((void **)&c.d_scratch, sizeof(double) * MK_MAXP * MK_NDOT));
    MK_HIP(hipMalloc((void **)&g_halt0, 2 * sizeof(int)));
    MK_HIP(hipMemset(g_halt0, 0, 2 * sizeof(int)));
    c.device = device;
    c.ready = true;
    return MK_OK;
}

static void mk_stager_release();                            // (staged host copies, below)

extern "C" int mk_shutdown(void) {
    MkContext &c = mk_ctx();
    if (!c.ready) return MK_OK;
    hipStreamSynchronize(c.stream);
    mk_stager_release();
    hipFree(g_halt0);
    g_halt0 = nullptr;
    hipFree(c.d_scratch);
    hipFree(c.pen_dump);
    c.pen_dump = nullptr;
    hipFree(c.arena);
    hipHostFree(c.h_scratch);
    hipStreamDestroy(c.stream);
    c = MkContext();
    return MK_OK;
}

extern "C" int mk_device_info(char *name, int *compute_units, size_t *hbm_bytes) {
    MK_REQUIRE_INIT();
    hipDeviceProp_t prop;
    MK_HIP(hipGetDeviceProperties(&prop, mk_ctx().device));
    if (name) snprintf(name, 256, "%s (%s)", prop.name, prop.gcnArchName);
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    return MK_OK;
}

extern "C" int mk_sync(void) {
    MK_REQUIRE_INIT();
    MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    return MK_OK;
}

// ======================================================================================
// memory
// ======================================================================================
extern "C" int mk_malloc(void **dptr, size_t bytes) {
    MK_REQUIRE_INIT();
    MK_ARG(dptr != nullptr);
    MK_HIP(hipMalloc(dptr, (bytes ? bytes : 16) + 16));     // slack: kernels read vectors in 16-byte pairs
    return MK_OK;
}

extern "C" int mk_free(void *dptr) {
    if (!dptr) return MK_OK;
    MK_REQUIRE_INIT();
    MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    MK_HIP(hipFree(dptr));
    return MK_OK;
}

// Large transfers between PAGEABLE host arrays (NumPy's) and the device.  hipMemcpy stages such a copy through
// pinned memory on one thread: 10-12 GB/s measured here (tools/setup_time.py), a second for the CSR arrays of a 512^3
// matrix.  Above 64 MiB the copy is cut into 16 MiB pieces that MK_COPY_THREADS (default 4) workers take in turn,
// each with its own pinned buffer and stream: host memcpy of one piece overlaps the DMA of the others.  Synchronous:
// the solver stream is drained first (the device side of the copy may be in use) and every worker waits for its own
// pieces, so on return the data is where it should be.
namespace {
constexpr size_t MK_COPY_PIECE = (size_t)16 << 20;
constexpr int MK_COPY_MAXT = 8;
struct MkStager {
    void *pin[MK_COPY_MAXT] = {};
    hipStream_t st[MK_COPY_MAXT] = {};
    int n = -1;                                              // -1: not tried yet, 0: unavailable
};
MkStager g_stager;

int stager_threads() {
    if (g_stager.n >= 0) return g_stager.n;
    static_assert(mk_switch_table[MK_SW_COPY_THREADS].hi == MK_COPY_MAXT, "one pinned buffer and stream per worker");
    const int want = (int)mk_switch_int<MK_SW_COPY_THREADS>();
    int got = 0;
    for (; got < want; ++got) {
        if (hipHostMalloc(&g_stager.pin[got], MK_COPY_PIECE, hipHostMallocDefault) != hipSuccess) break;
        if (hipStreamCreateWithFlags(&g_stager.st[got], hipStreamNonBlocking) != hipSuccess) {
            hipHostFree(g_stager.pin[got]);
            g_stager.pin[got] = nullptr;
            break;
        }
    }
    (void)hipGetLastError();
    g_stager.n = got < 2 ? 0 : got;                          // (one worker would only add a copy)
    return g_stager.n;
}

// returns MK_OK, or -1 when the caller should use the plain copy
std::mutex g_stager_mu;

int staged_copy(void *dst, const void *src, size_t bytes, bool h2d) {
    if (bytes < 4 * MK_COPY_PIECE) return -1;
    // ctypes releases the GIL: a second host thread that arrives while the pinned buffers are in use takes the plain copy
    std::unique_lock<std::mutex> hold(g_stager_mu, std::try_to_lock);
    if (!hold.owns_lock()) return -1;
    const int nt = stager_threads();
    if (nt == 0) return -1;
    if (hipStreamSynchronize(mk_ctx().stream) != hipSuccess) return -1;
    const int dev = mk_ctx().device;
    std::atomic<size_t> next{0};
    std::atomic<int> failed{0};
    auto work = [&](int k) {
        if (hipSetDevice(dev) != hipSuccess) {
            failed = 1;
            return;
        }
        for (;;) {
            const size_t off = next.fetch_add(MK_COPY_PIECE);
            if (off >= bytes || failed.load()) return;
            const size_t len = bytes - off < MK_COPY_PIECE ? bytes - off : MK_COPY_PIECE;
            bool ok;
            if (h2d) {
                memcpy(g_stager.pin[k], (const char *)src + off, len);
                ok = hipMemcpyAsync((char *)dst + off, g_stager.pin[k], len, hipMemcpyHostToDevice, g_stager.st[k]) == hipSuccess &&
                     hipStreamSynchronize(g_stager.st[k]) == hipSuccess;
            } else {
                ok = hipMemcpyAsync(g_stager.pin[k], (const char *)src + off, len, hipMemcpyDeviceToHost, g_stager.st[k]) == hipSuccess &&
                     hipStreamSynchronize(g_stager.st[k]) == hipSuccess;
                if (ok) memcpy((char *)dst + off, g_stager.pin[k], len);
            }
            if (!ok) failed = 1;
        }
    };
    std::thread th[MK_COPY_MAXT];
    for (int k = 1; k < nt; ++k) th[k] = std::thread(work, k);
    work(0);
    for (int k = 1; k < nt; ++k) th[k].join();
    if (failed.load()) return mk_fail(MK_ERR_HIP, "staged host copy of %zu bytes failed", bytes);
    return MK_OK;
}
}  // namespace

static void mk_stager_release() {
    for (int k = 0; k < MK_COPY_MAXT; ++k) {
        if (g_stager.st[k]) hipStreamDestroy(g_stager.st[k]);
        if (g_stager.pin[k]) hipHostFree(g_stager.pin[k]);
    }
    g_stager = MkStager();
}

// host -> device on the solver stream; large pageable sources take the staged path.  `sync`: wait for the copy.
int mk_upload(void *dst, const void *src, size_t bytes, bool sync) {
    if (!bytes) return MK_OK;
    const int rc = staged_copy(dst, src, bytes, true);
    if (rc >= 0) return rc;
    MK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, mk_ctx().stream));
    if (sync) MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    return MK_OK;
}

int mk_download(void *dst, const void *src, size_t bytes, bool sync) {
    if (!bytes) return MK_OK;
    const int rc = staged_copy(dst, src, bytes, false);
    if (rc >= 0) return rc;
    MK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, mk_ctx().stream));
    if (sync) MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    return MK_OK;
}

extern "C" int mk_memcpy_h2d(void *dst, const void *src, size_t bytes) {
    MK_REQUIRE_INIT();
    if (!bytes) return MK_OK;
    MK_ARG(dst && src);
    return mk_upload(dst, src, bytes, true);
}

extern "C" int mk_memcpy_d2h(void *dst, const void *src, size_t bytes) {
    MK_REQUIRE_INIT();
    if (!bytes) return MK_OK;
    MK_ARG(dst && src);
    return mk_download(dst, src, bytes, true);
}

extern "C" int mk_memcpy_d2d(void *dst, const void *src, size_t bytes) {
    MK_REQUIRE_INIT();
    if (!bytes) return MK_OK;
    MK_ARG(dst && src);
    MK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, mk_ctx().stream));
    return MK_OK;
}

extern "C" int mk_memset(void *dst, int byte, size_t bytes) {
    MK_REQUIRE_INIT();
    if (!bytes) return MK_OK;
    MK_ARG(dst != nullptr);
    MK_HIP(hipMemsetAsync(dst, byte, bytes, mk_ctx().stream));
    return MK_OK;
}

// ======================================================================================
// CSR container
// ======================================================================================
int mk_csr_alloc(int64_t nrows, int64_t ncols, int64_t nnz, mk_csr **out) {
    MK_ARG(out != nullptr);
    MK_ARG(nrows >= 0 && ncols >= 0 && nnz >= 0);
    if (nnz > 2147483647LL || ncols > 2147483647LL)
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr: nnz=%lld / ncols=%lld exceed the int32 index range",
                       (long long)nnz, (long long)ncols);
    mk_csr *A = new mk_csr();
    A->nrows = nrows;
    A->ncols = ncols;
    A->nnz = nnz;
    A->ntiles = (nrows + MK_ROWS_PER_TILE - 1) / MK_ROWS_PER_TILE;
    hipError_t e1 = hipMalloc((void **)&A->d_indptr, sizeof(int32_t) * (size_t)(nrows + 1));
    // +4 entries: the SpMV kernel reads nonzeros in aligned groups of four and may touch three slots past the end
    hipError_t e2 = hipMalloc((void **)&A->d_indices, sizeof(int32_t) * (size_t)(nnz + MK_CSR_PAD));
    hipError_t e3 = hipMalloc((void **)&A->d_data, sizeof(double) * (size_t)(nnz + MK_CSR_PAD));
    // (on the library's stream: the legacy default stream is not ordered with a non-blocking stream)
    if (e2 == hipSuccess) e2 = hipMemsetAsync(A->d_indices + nnz, 0, MK_CSR_PAD * sizeof(int32_t), mk_ctx().stream);
    if (e3 == hipSuccess) e3 = hipMemsetAsync(A->d_data + nnz, 0, MK_CSR_PAD * sizeof(double), mk_ctx().stream);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        mk_csr_destroy(A);
        return mk_fail(MK_ERR_HIP, "mk_csr: hipMalloc failed for nrows=%lld nnz=%lld", (long long)nrows,
                       (long long)nnz);
    }
    *out = A;
    return MK_OK;
}

extern "C" int mk_csr_create(int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *indptr,
                             const int32_t *indices, const double *data, mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(indptr != nullptr && (nnz == 0 || (indices && data)));
    MK_ARG(indptr[0] == 0 && (int64_t)indptr[nrows] == nnz);
    mk_csr *A = nullptr;
    int rc = mk_csr_alloc(nrows, ncols, nnz, &A);
    if (rc != MK_OK) return rc;
    hipStream_t st = mk_ctx().stream;
    MK_HIP(hipMemcpyAsync(A->d_indptr, indptr, sizeof(int32_t) * (size_t)(nrows + 1), hipMemcpyHostToDevice, st));
    if (nnz) {
        rc = mk_upload(A->d_indices, indices, sizeof(int32_t) * (size_t)nnz, false);
        if (rc == MK_OK) rc = mk_upload(A->d_data, data, sizeof(double) * (size_t)nnz, false);
        if (rc != MK_OK) {
            mk_csr_destroy(A);
            return rc;
        }
    }
    MK_HIP(hipStreamSynchronize(st));
    *out = A;
    return MK_OK;
}

extern "C" int mk_csr_compose(const mk_csr *A, int32_t nops, const mk_rowop *ops, mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(A != nullptr && out != nullptr && nops >= 0 && (nops == 0 || ops != nullptr));
    if (A->nops + nops > MK_ROWPROG_MAX)
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr_compose: at most %d steps per operator", (int)MK_ROWPROG_MAX);
    if (A->ex.mode >= 0)
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr_compose: compose before the operator is partitioned");
    if (A->comp_kind || A->host_fn)
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr_compose: the operand has no matrix of its own (sum / product / matrix-free)");
    for (int k = 0; k < nops; ++k) {
        MK_ARG(ops[k].code >= MK_ROW_SCALE && ops[k].code <= MK_ROW_RSUB);
        if (ops[k].code != MK_ROW_SCALE && A->nrows != A->ncols)
            return mk_fail(MK_ERR_ARG, "mk_csr_compose: adding a diagonal operator needs a square matrix");
    }
    mk_csr *B = new mk_csr(*A);
    B->alias = true;
    B->base = A->base ? A->base : A;
    B->plan = MkPlan();
    B->dependents = 0;
    B->doomed = false;
    B->base->dependents += 1;
    for (int k = 0; k < nops; ++k) B->ops[B->nops++] = ops[k];
    *out = B;
    return MK_OK;
}

static int pair_create(const mk_csr *A, const mk_csr *B, int kind, mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(A && B && out);
    if (!A->is_plain() || !B->is_plain())
        return mk_fail(MK_ERR_UNSUPPORTED, "operands of a device sum / product must be device matrices, with or without "
                                           "a row program (not sums / products / block operators, matrix-free or "
                                           "partitioned operators)");
    if (kind == 3) MK_ARG(A->ncols == B->nrows);
    else MK_ARG(A->nrows == B->nrows && A->ncols == B->ncols);
    mk_csr *C = new mk_csr();
    C->nrows = A->nrows;
    C->ncols = B->ncols;
    C->nnz = A->nnz + B->nnz;
    C->ntiles = (C->nrows + MK_ROWS_PER_TILE - 1) / MK_ROWS_PER_TILE;
    C->comp_kind = kind;
    C->comp_a = A;
    C->comp_b = B;
    C->plan.built = true;
    const int64_t tlen = (kind == 3) ? B->nrows : A->nrows;
    if (hipMalloc((void **)&C->d_comp_tmp, sizeof(double) * (size_t)(tlen > 0 ? tlen : 1) + 16) != hipSuccess ||
        hipMemsetAsync(C->d_comp_tmp, 0, sizeof(double) * (size_t)(tlen > 0 ? tlen : 1) + 16, mk_ctx().stream) != hipSuccess) {
        hipFree(C->d_comp_tmp);
        delete C;
        return mk_fail(MK_ERR_HIP, "device sum / product: allocation failed");
    }
    A->dependents += 1;
    B->dependents += 1;
    *out = C;
    return MK_OK;
}

// Block operators on the device.  The reference evaluates a block row as  y_i = 0 ; y_i += B_i0 * x_0 ; y_i += B_i1 * x_1 ...
// (blkop.py:86-96): every block product is a complete product of its own, and the results are added to the row's
// accumulator one block at a time.  Same here: one launch per block, whose row epilogue adds the finished row sum to the
// accumulator (the first block of a row adds to +0.0), then one launch that feeds the accumulated rows to the real
// epilogue of the calling kernel site (mk_device.h).  Blocks are borrowed handles of plain device matrices.
extern "C" int mk_csr_create_block(int32_t nbr, int32_t nbc, const mk_csr *const *blocks, const int64_t *heights,
                                   const int64_t *widths, mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(nbr >= 1 && nbc >= 1 && blocks && heights && widths && out);
    MkBlockGrid *G = new MkBlockGrid();
    G->nbr = nbr;
    G->nbc = nbc;
    G->roff.assign(nbr + 1, 0);
    G->coff.assign(nbc + 1, 0);
    for (int i = 0; i < nbr; ++i) G->roff[i + 1] = G->roff[i] + heights[i];
    for (int j = 0; j < nbc; ++j) G->coff[j + 1] = G->coff[j] + widths[j];
    int64_t nnz = 0, wmax = 1;
    bool ok = true, plain = true;
    for (int i = 0; i < nbr && ok; ++i)
        for (int j = 0; j < nbc && ok; ++j) {
            const mk_csr *B = blocks[i * nbc + j];
            G->blk.push_back(B);
            if (!B) continue;
            plain = plain && B->is_plain();
            ok = heights[i] >= 0 && widths[j] >= 0 && B->nrows == heights[i] && B->ncols == widths[j];
            nnz += B->nnz;
            wmax = B->ncols > wmax ? B->ncols : wmax;
        }
    if (!ok || !plain || G->roff[nbr] > 2147483647LL || G->coff[nbc] > 2147483647LL) {
        delete G;
        if (!plain)
            return mk_fail(MK_ERR_UNSUPPORTED, "blocks of a device block operator must be device matrices, with or without "
                                               "a row program (not composites, matrix-free or partitioned operators)");
        return mk_fail(MK_ERR_ARG, "mk_csr_create_block: block shapes do not fit the grid");
    }
    mk_csr *C = new mk_csr();
    C->nrows = G->roff[nbr];
    C->ncols = G->coff[nbc];
    C->nnz = nnz;
    C->ntiles = (C->nrows + MK_ROWS_PER_TILE - 1) / MK_ROWS_PER_TILE;
    C->comp_kind = 4;
    C->grid = G;
    C->plan.built = true;
    const size_t ybytes = sizeof(double) * (size_t)(C->nrows > 0 ? C->nrows : 1) + 16;
    if (hipMalloc((void **)&C->d_comp_tmp, ybytes) != hipSuccess ||
        hipMalloc((void **)&G->d_xtmp, sizeof(double) * (size_t)wmax + 16) != hipSuccess ||
        hipMemsetAsync(C->d_comp_tmp, 0, ybytes, mk_ctx().stream) != hipSuccess) {
        hipFree(C->d_comp_tmp);
        hipFree(G->d_xtmp);
        delete G;
        delete C;
        return mk_fail(MK_ERR_HIP, "mk_csr_create_block: allocation failed");
    }
    for (const mk_csr *B : G->blk)
        if (B) B->dependents += 1;
    *out = C;
    return MK_OK;
}

extern "C" int mk_csr_create_sum(const mk_csr *A, const mk_csr *B, int sign, mk_csr **out) {
    MK_ARG(sign == 1 || sign == -1);
    return pair_create(A, B, sign > 0 ? 1 : 2, out);
}

extern "C" int mk_csr_create_product(const mk_csr *A, const mk_csr *B, mk_csr **out) {
    return pair_create(A, B, 3, out);
}

extern "C" int mk_csr_create_callback(int64_t nrows, int64_t ncols, mk_matvec_fn fn, void *user, int transpose,
                                      mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(nrows >= 0 && ncols >= 0 && fn != nullptr && out != nullptr);
    MK_ARG(nrows <= 2147483647LL && ncols <= 2147483647LL);
    mk_csr *A = new mk_csr();
    A->nrows = nrows;
    A->ncols = ncols;
    A->nnz = 0;
    A->ntiles = (nrows + MK_ROWS_PER_TILE - 1) / MK_ROWS_PER_TILE;
    A->host_fn = fn;
    A->host_user = user;
    A->host_transpose = transpose;
    A->plan.built = true;
    const size_t nin = (size_t)(ncols > 0 ? ncols : 1), nout = (size_t)(nrows > 0 ? nrows : 1);
    if (hipHostMalloc((void **)&A->h_cb_in, sizeof(double) * nin, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&A->h_cb_out, sizeof(double) * nout, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&A->d_cb_in, sizeof(double) * nin + 16) != hipSuccess ||
        hipMalloc((void **)&A->d_cb_out, sizeof(double) * nout + 16) != hipSuccess ||
        hipMalloc((void **)&A->d_cb_go, sizeof(int)) != hipSuccess) {
        mk_csr_destroy(A);
        return mk_fail(MK_ERR_HIP, "mk_csr_create_callback: allocation failed for %lld x %lld", (long long)nrows,
                       (long long)ncols);
    }
    *out = A;
    return MK_OK;
}

// the host side of a matrix-free product: reads the gate's decision, and if the product is wanted copies the
// materialised input to the host, calls the operator, and puts the result where the epilogue launch reads it
int mk_host_product(const mk_csr *A, hipStream_t st) {
    int go = 0;
    MK_HIP(hipMemcpyAsync(&go, A->d_cb_go, sizeof(int), hipMemcpyDeviceToHost, st));
    MK_HIP(hipStreamSynchronize(st));
    if (!go) return MK_OK;                                   // loop condition failed (or halted): the reference would
                                                             // not have called `op * v` either
    if (A->ncols > 0)
        MK_HIP(hipMemcpyAsync(A->h_cb_in, A->d_cb_in, sizeof(double) * (size_t)A->ncols, hipMemcpyDeviceToHost, st));
    MK_HIP(hipStreamSynchronize(st));
    if (A->host_fn(A->host_user, A->host_transpose, A->h_cb_in, A->h_cb_out) != 0)
        return mk_fail(MK_ERR_STATE, "the host operator callback reported a failure");
    if (A->nrows > 0)
        MK_HIP(hipMemcpyAsync(A->d_cb_out, A->h_cb_out, sizeof(double) * (size_t)A->nrows, hipMemcpyHostToDevice, st));
    return MK_OK;
}

// Restriction of a device matrix to rows `rows` and columns `cols` (reference ReducedLinearOperator, linop.py:560-587:
// `z = zeros(n); z[col_indices] = x; return (op * z)[row_indices]`).  `cols` must not repeat an index (the reference's
// NumPy assignment would keep the last one; a parallel scatter has no "last").
extern "C" int mk_csr_create_reduced(const mk_csr *A, int64_t nrows, const int32_t *rows, int64_t ncols,
                                     const int32_t *cols, mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(A && out && nrows >= 0 && ncols >= 0 && (nrows == 0 || rows) && (ncols == 0 || cols));
    if (!A->is_plain())
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr_create_reduced: the operand must be a device matrix, with or without a "
                                           "row program (not a composite, matrix-free or partitioned operator)");
    for (int64_t i = 0; i < nrows; ++i) MK_ARG(rows[i] >= 0 && rows[i] < A->nrows);
    for (int64_t j = 0; j < ncols; ++j) MK_ARG(cols[j] >= 0 && cols[j] < A->ncols);
    mk_csr *C = new mk_csr();
    MkReduced *R = new MkReduced();
    C->nrows = nrows;
    C->ncols = ncols;
    C->nnz = A->nnz;
    C->ntiles = (nrows + MK_ROWS_PER_TILE - 1) / MK_ROWS_PER_TILE;
    C->comp_kind = 5;
    C->comp_a = A;
    C->red = R;
    C->plan.built = true;
    hipStream_t st = mk_ctx().stream;
    auto bytes = [](int64_t n, size_t w) { return w * (size_t)(n > 0 ? n : 1) + 16; };
    bool ok = hipMalloc((void **)&R->d_rows, bytes(nrows, 4)) == hipSuccess &&
              hipMalloc((void **)&R->d_cols, bytes(ncols, 4)) == hipSuccess &&
              hipMalloc((void **)&R->d_z, bytes(A->ncols, 8)) == hipSuccess &&
              hipMalloc((void **)&R->d_t, bytes(A->nrows, 8)) == hipSuccess &&
              hipMalloc((void **)&C->d_comp_tmp, bytes(nrows, 8)) == hipSuccess;
    if (ok && nrows) ok = hipMemcpyAsync(R->d_rows, rows, 4 * (size_t)nrows, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok && ncols) ok = hipMemcpyAsync(R->d_cols, cols, 4 * (size_t)ncols, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) ok = hipMemsetAsync(R->d_t, 0, bytes(A->nrows, 8), st) == hipSuccess &&
                 hipMemsetAsync(C->d_comp_tmp, 0, bytes(nrows, 8), st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) {
        hipFree(R->d_rows);
        hipFree(R->d_cols);
        hipFree(R->d_z);
        hipFree(R->d_t);
        hipFree(C->d_comp_tmp);
        delete R;
        delete C;
        return mk_fail(MK_ERR_HIP, "mk_csr_create_reduced: allocation failed");
    }
    A->dependents += 1;
    *out = C;
    return MK_OK;
}

// an operand loses one dependent; if its owner has destroyed it in the meantime, it goes now
void mk_release_operand(const mk_csr *B) {
    if (!B) return;
    B->dependents -= 1;
    if (B->dependents <= 0 && B->doomed) mk_csr_destroy(const_cast<mk_csr *>(B));
}

extern "C" int mk_csr_destroy(mk_csr *A) {
    if (!A) return MK_OK;
    if (A->dependents > 0) {                                 // composites still borrow its arrays: destroyed with the last
        A->doomed = true;
        return MK_OK;
    }
    if (A->alias) {
        const mk_csr *base = A->base;
        delete A;
        mk_release_operand(base);
        return MK_OK;
    }
    if (A->comp_kind) {
        if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
        hipFree(A->d_comp_tmp);
        const mk_csr *a = A->comp_a, *b = A->comp_b;
        MkBlockGrid *G = A->grid;
        if (A->red) {
            hipFree(A->red->d_rows);
            hipFree(A->red->d_cols);
            hipFree(A->red->d_z);
            hipFree(A->red->d_t);
            delete A->red;
        }
        delete A;
        mk_release_operand(a);
        mk_release_operand(b);
        if (G) {
            hipFree(G->d_xtmp);
            for (const mk_csr *B : G->blk) mk_release_operand(B);
            delete G;
        }
        return MK_OK;
    }
    if (A->host_fn) {
        if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
        if (A->h_cb_in) hipHostFree(A->h_cb_in);
        if (A->h_cb_out) hipHostFree(A->h_cb_out);
        hipFree(A->d_cb_in);
        hipFree(A->d_cb_out);
        hipFree(A->d_cb_go);
        delete A;
        return MK_OK;
    }
    if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
    mk_csr_plan_reset(A);
    hipFree(A->d_indptr);
    hipFree(A->d_indices);
    hipFree(A->d_data);
    hipFree(A->ex.d_send_idx);
    hipFree(A->ex.d_send_buf);
    hipFree(A->ex.d_tiles);
    if (A->ex.comm_stream) hipStreamDestroy(A->ex.comm_stream);
    if (A->ex.ev_pack) hipEventDestroy(A->ex.ev_pack);
    if (A->ex.ev_comm) hipEventDestroy(A->ex.ev_comm);
    if (A->ex.ev_comm0) hipEventDestroy(A->ex.ev_comm0);
    delete A;
    return MK_OK;
}

extern "C" int mk_csr_shape(const mk_csr *A, int64_t *nrows, int64_t *ncols, int64_t *nnz) {
    MK_ARG(A != nullptr);
    if (nrows) *nrows = A->nrows;
    if (ncols) *ncols = A->ncols;
    if (nnz) *nnz = A->nnz;
    return MK_OK;
}

// smallest and largest stored column index (2147483647 / -1 for a matrix without entries): the range check of a
// matrix that came from host arrays, done where the arrays already are instead of in two NumPy passes over them
static __global__ __launch_bounds__(MK_BLOCK) void col_range_kernel(int64_t nnz, const int32_t *__restrict__ idx,
                                                                    int *__restrict__ minmax) {
    int lo = 2147483647, hi = -1;
    for (int64_t j = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * MK_BLOCK) {
        const int c = idx[j];
        lo = c < lo ? c : lo;
        hi = c > hi ? c : hi;
    }
    atomicMin(&minmax[0], lo);
    atomicMax(&minmax[1], hi);
}

extern "C" int mk_csr_col_range(const mk_csr *A, int32_t *min_col, int32_t *max_col) {
    MK_REQUIRE_INIT();
    MK_ARG(A != nullptr);
    if (A->comp_kind || A->host_fn) return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr_col_range: the operand has no matrix of its own");
    int h_mm[2] = {2147483647, -1};
    if (A->nnz > 0) {
        hipStream_t st = mk_ctx().stream;
        int *d_mm = nullptr;
        MK_HIP(hipMalloc((void **)&d_mm, sizeof(h_mm)));
        bool ok = hipMemcpyAsync(d_mm, h_mm, sizeof(h_mm), hipMemcpyHostToDevice, st) == hipSuccess;
        int grid = (int)((A->nnz + MK_BLOCK - 1) / MK_BLOCK);
        grid = grid > 4096 ? 4096 : grid;
        if (ok) hipLaunchKernelGGL(col_range_kernel, dim3(grid), dim3(MK_BLOCK), 0, st, A->nnz, A->d_indices, d_mm);
        ok = ok && hipMemcpyAsync(h_mm, d_mm, sizeof(h_mm), hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess;
        hipFree(d_mm);
        if (!ok) return mk_fail(MK_ERR_HIP, "mk_csr_col_range: device pass failed");
    }
    if (min_col) *min_col = h_mm[0];
    if (max_col) *max_col = h_mm[1];
    return MK_OK;
}

extern "C" int mk_csr_download(const mk_csr *A, int32_t *indptr, int32_t *indices, double *data) {
    MK_REQUIRE_INIT();
    MK_ARG(A != nullptr);
    if (A->comp_kind || A->host_fn) return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr_download: the operand has no matrix of its own");
    if (A->nnz > 0 && (!A->d_indices || !A->d_data))         // (defensive: a matrix whose CSR arrays are gone cannot be read back)
        return mk_fail(MK_ERR_STATE, "%s: the CSR arrays of this matrix were released", __func__);
    hipStream_t st = mk_ctx().stream;
    if (indptr)
        MK_HIP(hipMemcpyAsync(indptr, A->d_indptr, sizeof(int32_t) * (size_t)(A->nrows + 1), hipMemcpyDeviceToHost, st));
    int rc = MK_OK;
    if (indices && A->nnz) rc = mk_download(indices, A->d_indices, sizeof(int32_t) * (size_t)A->nnz, false);
    if (rc == MK_OK && data && A->nnz) rc = mk_download(data, A->d_data, sizeof(double) * (size_t)A->nnz, false);
    if (rc != MK_OK) return rc;
    MK_HIP(hipStreamSynchronize(st));
    return MK_OK;
}

extern "C" int mk_csr_download_rows(const mk_csr *A, int64_t row_begin, int64_t row_end, int32_t *indptr,
                                    int32_t *indices, double *data) {
    MK_REQUIRE_INIT();
    MK_ARG(A != nullptr);
    MK_ARG(row_begin >= 0 && row_begin <= row_end && row_end <= A->nrows);
    if (A->comp_kind || A->host_fn)
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr_download_rows: the operand has no matrix of its own");
    if (A->nnz > 0 && (!A->d_indices || !A->d_data))         // (defensive: a matrix whose CSR arrays are gone cannot be read back)
        return mk_fail(MK_ERR_STATE, "%s: the CSR arrays of this matrix were released", __func__);
    hipStream_t st = mk_ctx().stream;
    int32_t ends[2] = {0, 0};
    MK_HIP(hipMemcpyAsync(&ends[0], A->d_indptr + row_begin, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MK_HIP(hipMemcpyAsync(&ends[1], A->d_indptr + row_end, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (indptr)
        MK_HIP(hipMemcpyAsync(indptr, A->d_indptr + row_begin, sizeof(int32_t) * (size_t)(row_end - row_begin + 1),
                              hipMemcpyDeviceToHost, st));
    MK_HIP(hipStreamSynchronize(st));
    const size_t cnt = (size_t)(ends[1] - ends[0]);
    int rc = MK_OK;
    if (indices && cnt) rc = mk_download(indices, A->d_indices + ends[0], sizeof(int32_t) * cnt, false);
    if (rc == MK_OK && data && cnt) rc = mk_download(data, A->d_data + ends[0], sizeof(double) * cnt, false);
    if (rc != MK_OK) return rc;
    MK_HIP(hipStreamSynchronize(st));
    return MK_OK;
}

// ======================================================================================
// standalone SpMV and BLAS-1
// ======================================================================================
static MkHalt never_halt() { return MkHalt{g_halt0, 0, 0}; }

extern "C" int mk_spmv(const mk_csr *A, const double *x, double *y) {
    MK_REQUIRE_INIT();
    MK_ARG(A && x && y);
    MK_ARG(MK_ALIGNED16(x) && MK_ALIGNED16(y));              // kernels read / write vectors in 16-byte pairs
    if (A->nrows == 0) return MK_OK;
    MkPlainEpi epi{y};
    mk_spmv_launch(A, mk_grid_spmv_for(A), mk_ctx().stream, x, epi, MkNoGate(), never_halt(), mk_ctx().d_scratch);
    MK_HIP(hipGetLastError());
    if (mk_ctx().pending_rc != MK_OK) {
        const int rc = mk_ctx().pending_rc;
        mk_ctx().pending_rc = MK_OK;
        return rc;
    }
    return MK_OK;
}

__global__ __launch_bounds__(MK_BLOCK) void mk_finalize_kernel(const double *part, int np, double *out, int do_sqrt) {
    __shared__ double s4[4];
    const double t = mk_total(part, np, s4);
    if (threadIdx.x == 0) out[0] = do_sqrt ? __dsqrt_rn(t) : t;
}

static int dot_impl(int64_t n, const double *x, const double *y, double *result, int do_sqrt) {
    MK_REQUIRE_INIT();
    MK_ARG(n >= 0 && result && (n == 0 || (x && y)));
    MK_ARG(MK_ALIGNED16(x) && MK_ALIGNED16(y));
    MkContext &c = mk_ctx();
    if (n == 0) {
        *result = 0.0;
        return MK_OK;
    }
    const int grid = mk_grid_stream(n);
    MkOpDot<0> op{x, y};
    hipLaunchKernelGGL(mk_stream_kernel<MkOpDot<0>>, dim3(grid), dim3(MK_BLOCK), 0, c.stream, op, n, never_halt(),
                       c.d_scratch);
    hipLaunchKernelGGL(mk_finalize_kernel, dim3(1), dim3(MK_BLOCK), 0, c.stream, c.d_scratch, grid,
                       c.d_scratch + MK_MAXP, do_sqrt);
    MK_HIP(hipMemcpyAsync(c.h_scratch, c.d_scratch + MK_MAXP, sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MK_HIP(hipStreamSynchronize(c.stream));
    *result = c.h_scratch[0];
    return MK_OK;
}

extern "C" int mk_dot(int64_t n, const double *x, const double *y, double *result) {
    return dot_impl(n, x, y, result, 0);
}

extern "C" int mk_nrm2(int64_t n, const double *x, double *result) { return dot_impl(n, x, x, result, 1); }

struct OpAxpby {   // y = alpha*x + beta*y  (mode 0), y += alpha*x (mode 1), x *= alpha (mode 2)
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *x;
    double *y;
    double alpha, beta;
    int mode;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ double f(double a, double b) const {
        if (mode == 1) return b + alpha * a;
        if (mode == 2) return b * alpha;
        return alpha * a + beta * b;
    }
    __device__ void pair(int64_t i, double *) {
        double2 a = (mode == 2) ? double2{0.0, 0.0} : mk_ld2(x, i);
        double2 b = mk_ld2(y, i);
        b.x = f(a.x, b.x);
        b.y = f(a.y, b.y);
        mk_st2(y, i, b);
    }
    __device__ void one(int64_t i, double *) { y[i] = f(mode == 2 ? 0.0 : x[i], y[i]); }
};

static int axpby_impl(int64_t n, double alpha, const double *x, double beta, double *y, int mode) {
    MK_REQUIRE_INIT();
    MK_ARG(n >= 0 && (n == 0 || y) && (n == 0 || mode == 2 || x));
    MK_ARG(MK_ALIGNED16(x) && MK_ALIGNED16(y));
    if (n == 0) return MK_OK;
    OpAxpby op{x, y, alpha, beta, mode};
    hipLaunchKernelGGL(mk_stream_kernel<OpAxpby>, dim3(mk_grid_stream(n)), dim3(MK_BLOCK), 0, mk_ctx().stream, op, n,
                       never_halt(), mk_ctx().d_scratch);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

extern "C" int mk_axpy(int64_t n, double alpha, const double *x, double *y) { return axpby_impl(n, alpha, x, 0.0, y, 1); }
extern "C" int mk_axpby(int64_t n, double alpha, const double *x, double beta, double *y) {
    return axpby_impl(n, alpha, x, beta, y, 0);
}
extern "C" int mk_scal(int64_t n, double alpha, double *x) { return axpby_impl(n, alpha, nullptr, 0.0, x, 2); }

// ======================================================================================
// synthetic matrices generated in HBM
// ======================================================================================
// number of stored entries in rows [0, r) of the 5-point m x m Laplacian
__host__ __device__ static inline int64_t p2d_prefix(int64_t r, int64_t m) {
    const int64_t n = m * m;
    int64_t c = 5 * r;
    c -= (r < m ? r : m);                                 // rows on the bottom edge (gy == 0)
    c -= (r > n - m ? r - (n - m) : 0);                   // rows on the top edge (gy == m-1)
    c -= (r + m - 1) / m;                                 // gx == 0
    c -= r / m;                                           // gx == m-1
    return c;
}

__global__ __launch_bounds__(MK_BLOCK) void gen_poisson2d(int64_t m, int64_t r_begin, int64_t r_end, int32_t *indptr,
                                                          int32_t *indices, double *data) {
    const int64_t base = p2d_prefix(r_begin, m);
    for (int64_t r = r_begin + (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r <= r_end;
         r += (int64_t)gridDim.x * MK_BLOCK) {
        int64_t p = p2d_prefix(r, m) - base;
        indptr[r - r_begin] = (int32_t)p;
        if (r == r_end) break;
        const int64_t gx = r % m, gy = r / m;
        if (gy > 0) { indices[p] = (int32_t)(r - m); data[p++] = -1.0; }
        if (gx > 0) { indices[p] = (int32_t)(r - 1); data[p++] = -1.0; }
        indices[p] = (int32_t)r; data[p++] = 4.0;
        if (gx < m - 1) { indices[p] = (int32_t)(r + 1); data[p++] = -1.0; }
        if (gy < m - 1) { indices[p] = (int32_t)(r + m); data[p++] = -1.0; }
    }
}

__host__ __device__ static inline int64_t p3d_prefix(int64_t r, int64_t nx, int64_t ny, int64_t nz) {
    const int64_t pl = nx * ny, n = pl * nz;
    const int64_t zc = r / pl, rem = r % pl;
    int64_t c = 7 * r;
    c -= (r < pl ? r : pl);                               // gz == 0
    c -= (r > n - pl ? r - (n - pl) : 0);                 // gz == nz-1
    c -= zc * nx + (rem < nx ? rem : nx);                 // gy == 0
    c -= zc * nx + (rem > pl - nx ? rem - (pl - nx) : 0); // gy == ny-1
    c -= (r + nx - 1) / nx;                               // gx == 0
    c -= r / nx;                                          // gx == nx-1
    return c;
}

__global__ __launch_bounds__(MK_BLOCK) void gen_poisson3d(int64_t nx, int64_t ny, int64_t nz, int64_t r_begin,
                                                          int64_t r_end, int32_t *indptr, int32_t *indices,
                                                          double *data) {
    const int64_t pl = nx * ny;
    const int64_t base = p3d_prefix(r_begin, nx, ny, nz);
    for (int64_t r = r_begin + (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r <= r_end;
         r += (int64_t)gridDim.x * MK_BLOCK) {
        int64_t p = p3d_prefix(r, nx, ny, nz) - base;
        indptr[r - r_begin] = (int32_t)p;
        if (r == r_end) break;
        const int64_t gx = r % nx, gy = (r / nx) % ny, gz = r / pl;
        if (gz > 0) { indices[p] = (int32_t)(r - pl); data[p++] = -1.0; }
        if (gy > 0) { indices[p] = (int32_t)(r - nx); data[p++] = -1.0; }
        if (gx > 0) { indices[p] = (int32_t)(r - 1); data[p++] = -1.0; }
        indices[p] = (int32_t)r; data[p++] = 6.0;
        if (gx < nx - 1) { indices[p] = (int32_t)(r + 1); data[p++] = -1.0; }
        if (gy < ny - 1) { indices[p] = (int32_t)(r + nx); data[p++] = -1.0; }
        if (gz < nz - 1) { indices[p] = (int32_t)(r + pl); data[p++] = -1.0; }
    }
}

extern "C" int mk_csr_poisson2d(int64_t m, int64_t row_begin, int64_t row_end, mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(m >= 1 && row_begin >= 0 && row_begin <= row_end && row_end <= m * m);
    const int64_t nnz = p2d_prefix(row_end, m) - p2d_prefix(row_begin, m);
    mk_csr *A = nullptr;
    int rc = mk_csr_alloc(row_end - row_begin, m * m, nnz, &A);
    if (rc != MK_OK) return rc;
    const int64_t rows = row_end - row_begin + 1;
    int grid = (int)((rows + MK_BLOCK - 1) / MK_BLOCK);
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(gen_poisson2d, dim3(grid), dim3(MK_BLOCK), 0, mk_ctx().stream, m, row_begin, row_end,
                       A->d_indptr, A->d_indices, A->d_data);
    MK_HIP(hipGetLastError());
    MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    *out = A;
    return MK_OK;
}

extern "C" int mk_csr_poisson3d(int64_t nx, int64_t ny, int64_t nz, int64_t row_begin, int64_t row_end,
                                mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && row_begin >= 0 && row_begin <= row_end && row_end <= nx * ny * nz);
    const int64_t nnz = p3d_prefix(row_end, nx, ny, nz) - p3d_prefix(row_begin, nx, ny, nz);
    mk_csr *A = nullptr;
    int rc = mk_csr_alloc(row_end - row_begin, nx * ny * nz, nnz, &A);
    if (rc != MK_OK) return rc;
    const int64_t rows = row_end - row_begin + 1;
    int grid = (int)((rows + MK_BLOCK - 1) / MK_BLOCK);
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(gen_poisson3d, dim3(grid), dim3(MK_BLOCK), 0, mk_ctx().stream, nx, ny, nz, row_begin, row_end,
                       A->d_indptr, A->d_indices, A->d_data);
    MK_HIP(hipGetLastError());
    MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    *out = A;
    return MK_OK;
}

// Variable-coefficient 7-point operator  -div(k grad u)  on the same grid, same sparsity (integer arrays identical to
// gen_poisson3d), Dirichlet boundary.  Cell field k(c) = 0.5 + u(c), u(c) a 53-bit uniform from a splitmix64 hash of
// the cell number; the entry between cells a and b is minus the harmonic mean h = ((2 ka) kb) / (ka + kb) (symmetric
// bit for bit), the diagonal is the sum over the six directions, in storage order (-z, -y, -x, +x, +y, +z), of h where
// the neighbour exists and of k(c) itself where it does not (the coefficient of the boundary face): strictly
// diagonally dominant on boundary rows, SPD, and practically every stored value distinct -- no value dictionary, no
// constant-coefficient shortcut applies: this is the matrix that exercises the CSR product proper.  NumPy twin in
// the test infrastructure: csr_ref.poisson3d_varcoef (bit-identical arrays, tests/test_gpu_varcoef.py).  (mk_cell_field:
// mk_internal.h -- the Lanczos start vector of mk_lanczos.hip is the same hash.)

__global__ __launch_bounds__(MK_BLOCK) void gen_poisson3d_varcoef(int64_t nx, int64_t ny, int64_t nz, uint64_t seed,
                                                                  int64_t r_begin, int64_t r_end, int32_t *indptr,
                                                                  int32_t *indices, double *data) {
    const int64_t pl = nx * ny;
    const int64_t base = p3d_prefix(r_begin, nx, ny, nz);
    for (int64_t r = r_begin + (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r <= r_end;
         r += (int64_t)gridDim.x * MK_BLOCK) {
        int64_t p = p3d_prefix(r, nx, ny, nz) - base;
        indptr[r - r_begin] = (int32_t)p;
        if (r == r_end) break;
        const int64_t gx = r % nx, gy = (r / nx) % ny, gz = r / pl;
        const double kc = mk_cell_field(r, seed);
        const bool have[6] = {gz > 0, gy > 0, gx > 0, gx < nx - 1, gy < ny - 1, gz < nz - 1};
        const int64_t off[6] = {-pl, -nx, -1, 1, nx, pl};
        double t[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            t[d] = kc;
            if (have[d]) {
                const double kb = mk_cell_field(r + off[d], seed);
                t[d] = ((2.0 * kc) * kb) / (kc + kb);
            }
        }
        const double diag = ((((t[0] + t[1]) + t[2]) + t[3]) + t[4]) + t[5];
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (have[d]) { indices[p] = (int32_t)(r + off[d]); data[p++] = -t[d]; }
        indices[p] = (int32_t)r; data[p++] = diag;
#pragma unroll
        for (int d = 3; d < 6; ++d)
            if (have[d]) { indices[p] = (int32_t)(r + off[d]); data[p++] = -t[d]; }
    }
}

extern "C" int mk_csr_poisson3d_varcoef(int64_t nx, int64_t ny, int64_t nz, uint64_t seed, int64_t row_begin,
                                        int64_t row_end, mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && row_begin >= 0 && row_begin <= row_end && row_end <= nx * ny * nz);
    const int64_t nnz = p3d_prefix(row_end, nx, ny, nz) - p3d_prefix(row_begin, nx, ny, nz);
    mk_csr *A = nullptr;
    int rc = mk_csr_alloc(row_end - row_begin, nx * ny * nz, nnz, &A);
    if (rc != MK_OK) return rc;
    const int64_t rows = row_end - row_begin + 1;
    int grid = (int)((rows + MK_BLOCK - 1) / MK_BLOCK);
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(gen_poisson3d_varcoef, dim3(grid), dim3(MK_BLOCK), 0, mk_ctx().stream, nx, ny, nz, seed, row_begin,
                       row_end, A->d_indptr, A->d_indices, A->d_data);
    MK_HIP(hipGetLastError());
    MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    *out = A;
    return MK_OK;
}

// 27-point box stencil on an nx x ny x nz grid (every cell coupled to the <= 26 cells of its 3 x 3 x 3 neighbourhood,
// columns ascending = (dz, dy, dx) lexicographic), the sparsity of HPCG's operator.  seed == 0: constant coefficients --
// -1.0 off the diagonal, 26.0 on it (HPCG's values).  seed != 0: the variable-coefficient twin of
// mk_csr_poisson3d_varcoef -- entry (a, b) = -h(a, b), h the harmonic mean of the two cells' hashed coefficients, the
// diagonal the left-to-right sum over the 26 directions, in column order, of h where the neighbour exists and of k(a)
// where it does not.  Symmetric bit for bit, weakly diagonally dominant with strict rows on the boundary: SPD.
// Rows of 8 ... 27 entries: the matrix class of the wide storage formats (mk_format.hip).  NumPy twin: csr_ref.stencil27.
__host__ __device__ static inline int64_t s27_line(int64_t g, int64_t n) {      // sum over x < g of the cells x - 1 .. x + 1 inside
    return g + (g > 0 ? g - 1 : 0) + (g < n - 1 ? g : n - 1);
}
__host__ __device__ static inline int64_t s27_cnt(int64_t g, int64_t n) { return 1 + (g > 0 ? 1 : 0) + (g < n - 1 ? 1 : 0); }
__host__ __device__ static inline int64_t s27_prefix(int64_t r, int64_t nx, int64_t ny, int64_t nz) {
    const int64_t pl = nx * ny;
    if (r >= pl * nz) return s27_line(nx, nx) * s27_line(ny, ny) * s27_line(nz, nz);
    const int64_t gx = r % nx, gy = (r / nx) % ny, gz = r / pl;
    const int64_t SX = s27_line(nx, nx), SY = s27_line(ny, ny);
    return s27_line(gz, nz) * SY * SX + s27_cnt(gz, nz) * (s27_line(gy, ny) * SX + s27_cnt(gy, ny) * s27_line(gx, nx));
}

__global__ __launch_bounds__(MK_BLOCK) void gen_stencil27(int64_t nx, int64_t ny, int64_t nz, uint64_t seed, int64_t r_begin,
                                                          int64_t r_end, int32_t *indptr, int32_t *indices, double *data) {
    const int64_t pl = nx * ny;
    const int64_t base = s27_prefix(r_begin, nx, ny, nz);
    for (int64_t r = r_begin + (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r <= r_end;
         r += (int64_t)gridDim.x * MK_BLOCK) {
        int64_t p = s27_prefix(r, nx, ny, nz) - base;
        indptr[r - r_begin] = (int32_t)p;
        if (r == r_end) break;
        const int64_t gx = r % nx, gy = (r / nx) % ny, gz = r / pl;
        const double kc = seed ? mk_cell_field(r, seed) : 1.0;
        double diag = 0.0;
        int64_t pdiag = -1;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const bool self = (dz == 0 && dy == 0 && dx == 0);
                    const bool have = gz + dz >= 0 && gz + dz < nz && gy + dy >= 0 && gy + dy < ny && gx + dx >= 0 && gx + dx < nx;
                    const int64_t c = r + dz * pl + dy * nx + dx;
                    if (self) {
                        pdiag = p;
                        indices[p++] = (int32_t)r;
                        continue;
                    }
                    double h = kc;
                    if (have && seed) {
                        const double kb = mk_cell_field(c, seed);
                        h = ((2.0 * kc) * kb) / (kc + kb);
                    }
                    diag += h;
                    if (have) {
                        indices[p] = (int32_t)c;
                        data[p++] = -h;
                    }
                }
        data[pdiag] = diag;
    }
}

extern "C" int mk_csr_stencil27(int64_t nx, int64_t ny, int64_t nz, uint64_t seed, int64_t row_begin, int64_t row_end,
                                mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(out != nullptr && nx >= 1 && ny >= 1 && nz >= 1 && row_begin >= 0 && row_begin <= row_end && row_end <= nx * ny * nz);
    const int64_t nnz = s27_prefix(row_end, nx, ny, nz) - s27_prefix(row_begin, nx, ny, nz);
    if (nnz > (int64_t)0x7fffffff - MK_CSR_PAD) return mk_fail(MK_ERR_ARG, "mk_csr_stencil27: %lld nonzeros do not fit int32 row pointers", (long long)nnz);
    mk_csr *A = nullptr;
    int rc = mk_csr_alloc(row_end - row_begin, nx * ny * nz, nnz, &A);
    if (rc != MK_OK) return rc;
    const int64_t rows = row_end - row_begin + 1;
    int grid = (int)((rows + MK_BLOCK - 1) / MK_BLOCK);
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(gen_stencil27, dim3(grid), dim3(MK_BLOCK), 0, mk_ctx().stream, nx, ny, nz, seed, row_begin, row_end,
                       A->d_indptr, A->d_indices, A->d_data);
    MK_HIP(hipGetLastError());
    MK_HIP(hipStreamSynchronize(mk_ctx().stream));
    *out = A;
    return MK_OK;
}

// ======================================================================================
// transpose (K1T support): B = A^T with rows of B sorted by original row index
// ======================================================================================
__global__ __launch_bounds__(MK_BLOCK) void tr_count(int64_t nnz, const int32_t *indices, int32_t *count) {
    for (int64_t j = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * MK_BLOCK)
        atomicAdd(&count[indices[j] + 1], 1);
}

__global__ __launch_bounds__(MK_BLOCK) void tr_scatter(int64_t nrows, const int32_t *indptr, const int32_t *indices,
                                                       const double *data, int32_t *cursor, int32_t *t_indices,
                                                       double *t_data) {
    for (int64_t r = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * MK_BLOCK)
        for (int32_t j = indptr[r]; j < indptr[r + 1]; ++j) {
            const int32_t dst = atomicAdd(&cursor[indices[j]], 1);
            t_indices[dst] = (int32_t)r;
            t_data[dst] = data[j];
        }
}

// arrival order of the atomics is arbitrary: restore ascending original-row order per segment
__global__ __launch_bounds__(MK_BLOCK) void tr_sort_segments(int64_t ncols, const int32_t *t_indptr, int32_t *t_indices,
                                                             double *t_data) {
    for (int64_t c = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; c < ncols; c += (int64_t)gridDim.x * MK_BLOCK) {
        const int32_t lo = t_indptr[c], hi = t_indptr[c + 1];
        for (int32_t i = lo + 1; i < hi; ++i) {
            const int32_t ki = t_indices[i];
            const double vi = t_data[i];
            int32_t j = i - 1;
            while (j >= lo && t_indices[j] > ki) {
                t_indices[j + 1] = t_indices[j];
                t_data[j + 1] = t_data[j];
                --j;
            }
            t_indices[j + 1] = ki;
            t_data[j + 1] = vi;
        }
    }
}

constexpr int32_t MK_TR_DEVICE_MAX_COLUMN = 2048;     // longest column the device path sorts (one lane, insertion sort)

// (a failure after B exists frees it -- and the cursor array -- before returning: ADVICE r2)
#define MK_TR(expr)                                                                                \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            hipFree(cursor);                                                                       \
            mk_csr_destroy(B);                                                                     \
            return mk_fail(MK_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                          \
    } while (0)
extern "C" int mk_csr_transpose(const mk_csr *A, mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(A && out);
    if (A->comp_kind || A->host_fn)
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr_transpose: the operand has no matrix of its own; transpose its parts");
    if (A->nnz > 0 && (!A->d_indices || !A->d_data))         // (defensive: a matrix whose CSR arrays are gone cannot be read back)
        return mk_fail(MK_ERR_STATE, "%s: the CSR arrays of this matrix were released", __func__);
    mk_csr *B = nullptr;
    int32_t *cursor = nullptr;
    int rc = mk_csr_alloc(A->ncols, A->nrows, A->nnz, &B);
    if (rc != MK_OK) return rc;
    hipStream_t st = mk_ctx().stream;
    const size_t pbytes = sizeof(int32_t) * (size_t)(A->ncols + 1);
    MK_TR(hipMemsetAsync(B->d_indptr, 0, pbytes, st));
    int g1 = (int)((A->nnz + MK_BLOCK - 1) / MK_BLOCK);
    g1 = g1 < 1 ? 1 : (g1 > 65536 ? 65536 : g1);
    hipLaunchKernelGGL(tr_count, dim3(g1), dim3(MK_BLOCK), 0, st, A->nnz, A->d_indices, B->d_indptr);
    // exclusive scan of the column counts on the host (one-off, ncols ints)
    std::vector<int32_t> h((size_t)A->ncols + 1);
    MK_TR(hipMemcpyAsync(h.data(), B->d_indptr, pbytes, hipMemcpyDeviceToHost, st));
    MK_TR(hipStreamSynchronize(st));
    int32_t longest = 0;
    for (int64_t c = 0; c < A->ncols; ++c) {
        longest = h[c + 1] > longest ? h[c + 1] : longest;
        h[c + 1] += h[c];
    }
    MK_TR(hipMemcpyAsync(B->d_indptr, h.data(), pbytes, hipMemcpyHostToDevice, st));
    if (longest > MK_TR_DEVICE_MAX_COLUMN) {
        // A column this long (dense columns of least-squares / LP matrices) would make the per-segment insertion
        // sort below quadratic on ONE lane.  Such matrices are transposed by a stable counting sort on the host:
        // rows are visited in ascending order, so every transposed row comes out sorted by original row.
        std::vector<int32_t> ip((size_t)A->nrows + 1), ix((size_t)A->nnz), tix((size_t)A->nnz);
        std::vector<double> dv((size_t)A->nnz), tdv((size_t)A->nnz);
        MK_TR(hipMemcpyAsync(ip.data(), A->d_indptr, sizeof(int32_t) * ip.size(), hipMemcpyDeviceToHost, st));
        MK_TR(hipMemcpyAsync(ix.data(), A->d_indices, sizeof(int32_t) * ix.size(), hipMemcpyDeviceToHost, st));
        MK_TR(hipMemcpyAsync(dv.data(), A->d_data, sizeof(double) * dv.size(), hipMemcpyDeviceToHost, st));
        MK_TR(hipStreamSynchronize(st));
        std::vector<int32_t> cur(h.begin(), h.end() - 1);
        for (int64_t r = 0; r < A->nrows; ++r)
            for (int32_t j = ip[r]; j < ip[r + 1]; ++j) {
                const int32_t dst = cur[ix[j]]++;
                tix[dst] = (int32_t)r;
                tdv[dst] = dv[j];
            }
        MK_TR(hipMemcpyAsync(B->d_indices, tix.data(), sizeof(int32_t) * tix.size(), hipMemcpyHostToDevice, st));
        MK_TR(hipMemcpyAsync(B->d_data, tdv.data(), sizeof(double) * tdv.size(), hipMemcpyHostToDevice, st));
        MK_TR(hipStreamSynchronize(st));
        B->nops = A->nops;
        for (int k = 0; k < A->nops; ++k) B->ops[k] = A->ops[k];
        *out = B;
        return MK_OK;
    }
    MK_TR(hipMalloc((void **)&cursor, pbytes));
    MK_TR(hipMemcpyAsync(cursor, h.data(), pbytes, hipMemcpyHostToDevice, st));
    int g2 = (int)((A->nrows + MK_BLOCK - 1) / MK_BLOCK);
    g2 = g2 < 1 ? 1 : (g2 > 65536 ? 65536 : g2);
    hipLaunchKernelGGL(tr_scatter, dim3(g2), dim3(MK_BLOCK), 0, st, A->nrows, A->d_indptr, A->d_indices, A->d_data,
                       cursor, B->d_indices, B->d_data);
    int g3 = (int)((A->ncols + MK_BLOCK - 1) / MK_BLOCK);
    g3 = g3 < 1 ? 1 : (g3 > 65536 ? 65536 : g3);
    hipLaunchKernelGGL(tr_sort_segments, dim3(g3), dim3(MK_BLOCK), 0, st, A->ncols, B->d_indptr, B->d_indices,
                       B->d_data);
    MK_TR(hipGetLastError());
    MK_TR(hipStreamSynchronize(st));
    MK_TR(hipFree(cursor));
    // (alpha A + D)^T = alpha A^T + D: the row program of a composed operator carries over unchanged
    B->nops = A->nops;
    for (int k = 0; k < A->nops; ++k) B->ops[k] = A->ops[k];
    *out = B;
    return MK_OK;
}

// ======================================================================================
// coordinate triples -> canonical CSR on the device (the on-disk side of the path: MatrixMarket files and
// the reference's CoordLinearOperator, linop.py:638-685).  Integer work is done with integer atomics (their
// RESULT is order independent); the floating-point sums of duplicate entries are formed by one thread per
// row, sequentially, in input order -- so the arrays are bit-identical to a stable host sort + np.add.at.
// ======================================================================================
__global__ __launch_bounds__(MK_BLOCK) void coo_count(int64_t ne, const int32_t *rows, int32_t *count) {
    for (int64_t j = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; j < ne; j += (int64_t)gridDim.x * MK_BLOCK)
        atomicAdd(&count[rows[j] + 1], 1);
}

// an entry's key: its column above its position in the input list (both < 2^31), so that the order of the keys is the
// order by (column, input position)
__global__ __launch_bounds__(MK_BLOCK) void coo_scatter(int64_t ne, const int32_t *rows, const int32_t *cols,
                                                        int32_t *cursor, unsigned long long *seg_key) {
    for (int64_t j = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; j < ne; j += (int64_t)gridDim.x * MK_BLOCK) {
        const int32_t dst = atomicAdd(&cursor[rows[j]], 1);
        seg_key[dst] = ((unsigned long long)(uint32_t)cols[j] << 32) | (unsigned long long)j;
    }
}

// the keys of one row in ascending order, in place, by one lane: heapsort, for the rows an insertion sort would take
// quadratic time on (the expanded rows of the sparse products of mk_amg.hip hold thousands of entries)
__device__ __forceinline__ void coo_heap_sift(unsigned long long *key, int32_t root, int32_t size) {
    const unsigned long long k = key[root];
    for (int32_t child = 2 * root + 1; child < size; child = 2 * root + 1) {
        unsigned long long kc = key[child];
        if (child + 1 < size) {
            const unsigned long long k2 = key[child + 1];
            if (k2 > kc) {
                kc = k2;
                ++child;
            }
        }
        if (k >= kc) break;
        key[root] = kc;
        root = child;
    }
    key[root] = k;
}

constexpr int32_t MK_COO_INSERTION_MAX = 32;   // longest row the insertion sort takes

// per row: order by (column, input position) -- a total order, so neither the arbitrary arrival order of the scatter nor the
// sorting method matters -- and count the distinct columns
__global__ __launch_bounds__(MK_BLOCK) void coo_sort_rows(int64_t nrows, const int32_t *start, unsigned long long *seg_key,
                                                          int32_t *ucount) {
    for (int64_t r = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * MK_BLOCK) {
        const int32_t lo = start[r], hi = start[r + 1];
        if (hi - lo > MK_COO_INSERTION_MAX) {
            unsigned long long *const key = seg_key + lo;
            const int32_t size = hi - lo;
            for (int32_t root = size / 2 - 1; root >= 0; --root) coo_heap_sift(key, root, size);
            for (int32_t end = size - 1; end > 0; --end) {
                const unsigned long long top = key[0];
                key[0] = key[end];
                key[end] = top;
                coo_heap_sift(key, 0, end);
            }
        } else {
            for (int32_t i = lo + 1; i < hi; ++i) {
                const unsigned long long ki = seg_key[i];
                int32_t j = i - 1;
                while (j >= lo && seg_key[j] > ki) {
                    seg_key[j + 1] = seg_key[j];
                    --j;
                }
                seg_key[j + 1] = ki;
            }
        }
        int32_t u = 0;
        for (int32_t i = lo; i < hi; ++i) u += (i == lo || (seg_key[i] >> 32) != (seg_key[i - 1] >> 32)) ? 1 : 0;
        ucount[r + 1] = u;
    }
}

__global__ __launch_bounds__(MK_BLOCK) void coo_emit(int64_t nrows, const int32_t *start, const unsigned long long *seg_key,
                                                     const double *vals, const int32_t *indptr, int32_t *indices, double *data) {
    for (int64_t r = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * MK_BLOCK) {
        const int32_t lo = start[r], hi = start[r + 1];
        int32_t out = indptr[r] - 1;
        double sum = 0.0;
        for (int32_t i = lo; i < hi; ++i) {
            const unsigned long long k = seg_key[i];
            if (i == lo || (k >> 32) != (seg_key[i - 1] >> 32)) {
                if (i != lo) data[out] = sum;
                ++out;
                indices[out] = (int32_t)(k >> 32);
                sum = 0.0;
            }
            sum = sum + vals[(uint32_t)k];                  // duplicates: added in input order, starting from 0.0
        }
        if (hi > lo) data[out] = sum;
    }
}

static inline int mk_grid_for(int64_t n) {
    int64_t g = (n + MK_BLOCK - 1) / MK_BLOCK;
    return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

// The device half: coordinate lists already in device memory (rows in [0, nrows), columns in [0, ncols), nentries < 2^31)
// and the row starts of the list on the host (start[r + 1] - start[r] = entries of row r, nrows + 1 ints) -> canonical CSR.
// Scatter by row, per-row sort by (column, list position), emit with the duplicates summed in list order from 0.0.  Also the
// compress step of the sparse products of mk_amg.hip, whose expanded lists are formed on the device.  Synchronises.
int mk_coo_compress_device(int64_t nrows, int64_t ncols, int64_t nentries, const int32_t *d_rows, const int32_t *d_cols,
                           const double *d_vals, const int32_t *start_host, mk_csr **out) {
    hipStream_t st = mk_ctx().stream;
    const size_t pb = sizeof(int32_t) * (size_t)(nrows + 1), eb = sizeof(int32_t) * (size_t)(nentries ? nentries : 1);
    int32_t *d_start = nullptr, *d_cursor = nullptr, *d_ucount = nullptr;
    unsigned long long *d_key = nullptr;
    mk_csr *A = nullptr;
    int rc = MK_OK;
    auto cleanup = [&]() {
        hipFree(d_start); hipFree(d_cursor); hipFree(d_key); hipFree(d_ucount);
    };
#define MK_TRY(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            cleanup();                                                                                 \
            mk_csr_destroy(A);                                                                         \
            return mk_fail(MK_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));                 \
        }                                                                                              \
    } while (0)
    MK_TRY(hipMalloc((void **)&d_key, 2 * eb));
    MK_TRY(hipMalloc((void **)&d_start, pb));
    MK_TRY(hipMalloc((void **)&d_cursor, pb));
    MK_TRY(hipMalloc((void **)&d_ucount, pb));
    MK_TRY(hipMemcpyAsync(d_start, start_host, pb, hipMemcpyHostToDevice, st));
    MK_TRY(hipMemcpyAsync(d_cursor, start_host, pb, hipMemcpyHostToDevice, st));
    MK_TRY(hipMemsetAsync(d_ucount, 0, pb, st));
    if (nentries)
        hipLaunchKernelGGL(coo_scatter, dim3(mk_grid_for(nentries)), dim3(MK_BLOCK), 0, st, nentries, d_rows, d_cols,
                           d_cursor, d_key);
    if (nrows)
        hipLaunchKernelGGL(coo_sort_rows, dim3(mk_grid_for(nrows)), dim3(MK_BLOCK), 0, st, nrows, d_start, d_key,
                           d_ucount);
    std::vector<int32_t> u((size_t)nrows + 1, 0);
    MK_TRY(hipMemcpyAsync(u.data(), d_ucount, pb, hipMemcpyDeviceToHost, st));
    MK_TRY(hipStreamSynchronize(st));
    for (int64_t r = 0; r < nrows; ++r) u[r + 1] += u[r];
    rc = mk_csr_alloc(nrows, ncols, u[(size_t)nrows], &A);
    if (rc != MK_OK) {
        cleanup();
        return rc;
    }
    MK_TRY(hipMemcpyAsync(A->d_indptr, u.data(), pb, hipMemcpyHostToDevice, st));
    if (nrows)
        hipLaunchKernelGGL(coo_emit, dim3(mk_grid_for(nrows)), dim3(MK_BLOCK), 0, st, nrows, d_start, d_key,
                           d_vals, A->d_indptr, A->d_indices, A->d_data);
    MK_TRY(hipGetLastError());
    MK_TRY(hipStreamSynchronize(st));
#undef MK_TRY
    cleanup();
    *out = A;
    return MK_OK;
}

extern "C" int mk_csr_from_coo(int64_t nrows, int64_t ncols, int64_t nentries, const int32_t *rows,
                               const int32_t *cols, const double *vals, mk_csr **out) {
    MK_REQUIRE_INIT();
    MK_ARG(out && nrows >= 0 && ncols >= 0 && nentries >= 0 && (nentries == 0 || (rows && cols && vals)));
    if (nentries > 2147483647LL || ncols > 2147483647LL || nrows > 2147483646LL)
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr_from_coo: sizes exceed the int32 index range");
    std::vector<int32_t> h((size_t)nrows + 1, 0);
    for (int64_t j = 0; j < nentries; ++j) {
        if (rows[j] < 0 || rows[j] >= nrows || cols[j] < 0 || cols[j] >= ncols)
            return mk_fail(MK_ERR_ARG, "mk_csr_from_coo: entry %lld = (%d, %d) outside a %lld x %lld matrix",
                           (long long)j, rows[j], cols[j], (long long)nrows, (long long)ncols);
        h[(size_t)rows[j] + 1] += 1;
    }
    int32_t longest = 0;
    for (int64_t r = 0; r < nrows; ++r) {
        longest = h[r + 1] > longest ? h[r + 1] : longest;
        h[r + 1] += h[r];
    }
    if (longest > 16384)
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_csr_from_coo: a row with %d entries is too long for the per-row "
                       "device sort; build the CSR arrays on the host (mk_csr_create)", (int)longest);
    hipStream_t st = mk_ctx().stream;
    const size_t eb = sizeof(int32_t) * (size_t)(nentries ? nentries : 1);
    int32_t *d_rows = nullptr, *d_cols = nullptr;
    double *d_vals = nullptr;
    auto cleanup = [&]() {
        hipFree(d_rows); hipFree(d_cols); hipFree(d_vals);
    };
#define MK_TRY(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            cleanup();                                                                                 \
            return mk_fail(MK_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));                 \
        }                                                                                              \
    } while (0)
    MK_TRY(hipMalloc((void **)&d_rows, eb));
    MK_TRY(hipMalloc((void **)&d_cols, eb));
    MK_TRY(hipMalloc((void **)&d_vals, sizeof(double) * (size_t)(nentries ? nentries : 1)));
    if (nentries) {
        MK_TRY(hipMemcpyAsync(d_rows, rows, sizeof(int32_t) * (size_t)nentries, hipMemcpyHostToDevice, st));
        MK_TRY(hipMemcpyAsync(d_cols, cols, sizeof(int32_t) * (size_t)nentries, hipMemcpyHostToDevice, st));
        MK_TRY(hipMemcpyAsync(d_vals, vals, sizeof(double) * (size_t)nentries, hipMemcpyHostToDevice, st));
    }
#undef MK_TRY
    const int rc = mk_coo_compress_device(nrows, ncols, nentries, d_rows, d_cols, d_vals, h.data(), out);
    cleanup();
    return rc;
}

// ======================================================================================
// counter calibration helpers (profiles/: known byte counts at the access widths the solver
// kernels use, to scale rocprofv3's FETCH_SIZE / WRITE_SIZE on gfx950 -- MI355X_MICROARCH.md, HBM)
// ======================================================================================
template <typename T>
__global__ __launch_bounds__(MK_BLOCK) void calib_read_kernel(const T *__restrict__ p, int64_t count, double *sink) {
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; i < count; i += (int64_t)gridDim.x * MK_BLOCK) {
        const T v = p[i];
        if constexpr (sizeof(T) == 16) acc += v.x + v.y;
        else acc += (double)v;
    }
    if (acc == 1.2345e300) sink[0] = acc;       // never true: keeps the loads alive
}

template <typename T>
__global__ __launch_bounds__(MK_BLOCK) void calib_write_kernel(T *__restrict__ p, int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; i < count; i += (int64_t)gridDim.x * MK_BLOCK) {
        if constexpr (sizeof(T) == 16) p[i] = T{1.0, 2.0};
        else p[i] = (T)1;
    }
}

extern "C" int mk_calib_stream(void *dev, int64_t bytes, int width, int write) {
    MK_REQUIRE_INIT();
    MK_ARG(dev && bytes > 0 && (width == 4 || width == 8 || width == 16));
    hipStream_t st = mk_ctx().stream;
    const int grid = MK_MAXP * 2;
    const int64_t count = bytes / width;
    if (write) {
        if (width == 4) hipLaunchKernelGGL(calib_write_kernel<int32_t>, dim3(grid), dim3(MK_BLOCK), 0, st, (int32_t *)dev, count);
        if (width == 8) hipLaunchKernelGGL(calib_write_kernel<double>, dim3(grid), dim3(MK_BLOCK), 0, st, (double *)dev, count);
        if (width == 16) hipLaunchKernelGGL(calib_write_kernel<double2>, dim3(grid), dim3(MK_BLOCK), 0, st, (double2 *)dev, count);
    } else {
        double *sink = mk_ctx().d_scratch;
        if (width == 4) hipLaunchKernelGGL(calib_read_kernel<int32_t>, dim3(grid), dim3(MK_BLOCK), 0, st, (const int32_t *)dev, count, sink);
        if (width == 8) hipLaunchKernelGGL(calib_read_kernel<double>, dim3(grid), dim3(MK_BLOCK), 0, st, (const double *)dev, count, sink);
        if (width == 16) hipLaunchKernelGGL(calib_read_kernel<double2>, dim3(grid), dim3(MK_BLOCK), 0, st, (const double2 *)dev, count, sink);
    }
    MK_HIP(hipGetLastError());
    MK_HIP(hipStreamSynchronize(st));
    return MK_OK;
}
