// mk_solver.h -- host-side driver shared by all device-resident solver loops.
//
// A solver is a fixed sequence of kernels per pass of the reference's `while` body.  The
// host only enqueues; scalars (alpha, beta, rotations, norms, stop tests) live in device
// memory and are recomputed by every workgroup from the previous kernel's partial sums, so
// there is no device->host round trip inside an iteration.  The driver enqueues a batch of
// iterations, then reads back one small status record to learn whether the loop condition
// failed (kernels after that point are no-ops thanks to MkHalt).
#pragma once
#include "mk_device.h"

struct MkStatus {            // lives in device memory, written by one lane only
    int64_t nMatvec;
    int64_t itn;
    int64_t hist_len;
    int32_t istop;
    int32_t definite;
    int32_t converged;
    int32_t pad;
};

constexpr int64_t MK_HIST_RING = 1 << 16;   // residual-history ring (drained after every batch)
constexpr int64_t MK_BATCH_MAX = 256;

// Collective hooks (implemented in mk_comm.hip; no-ops without a communicator).
int mk_comm_active();
int mk_comm_allreduce_sum(double *buf_dev, int64_t count, hipStream_t stream);
int mk_comm_reduce_scatter_sum(const double *full_dev, double *mine_dev, int64_t count_per_rank, hipStream_t stream);
int mk_comm_allgather(const double *mine_dev, double *full_dev, int64_t count_per_rank, hipStream_t stream);
int mk_exchange_begin(const mk_csr *A, double *x_ext);     // may leave the messages in flight on a second stream
int mk_exchange_wait(const mk_csr *A, hipStream_t stream); // ... until here

// A device object that applies out = P in by launches of its own, inside a solver's loop under the loop's halt words or
// standalone.  What every kind shares is here: the row count, the count of its holders (a solver that applies the object holds
// it; destroying it meanwhile is deferred to the last release), the two never-raised halt words of a launch outside a loop,
// and the standalone apply behind mk_<kind>_apply.  A kind derives from it, gives `enqueue` and `noun`, calls `init_nohalt`
// in its create path before its first launch, and frees its own device memory in its destructor (after draining the stream;
// the base destructor then frees the words).
struct MkDeviceOp {
    int64_t n = 0;                 // rows
    mutable int users = 0;         // solvers holding the object
    mutable bool doomed = false;   // `destroy` was called while solvers still held it
    int *d_nohalt = nullptr;       // two zero words (owned): the halt input of a launch that no loop can halt
    virtual ~MkDeviceOp() { hipFree(d_nohalt); }
    // what the object is, for the messages of the setters: "the <noun> has ... rows"
    virtual const char *noun() const = 0;
    // out = P in on `stream` (in == out allowed); every launch takes `halt(flags, q)`
    virtual int enqueue(const double *in, double *out, hipStream_t stream, int *flags, int64_t *q) const = 0;
    // allocates the two words and zeroes them in stream order
    int init_nohalt(hipStream_t stream);
    // the halt words of the next launch: flags[(*q)++ & 1] of the loop whose kernel counter is `q`, or, q null (a standalone
    // run, the object's own set-up), the words that are never raised
    MkHalt halt(int *flags, int64_t *q) const { return q ? MkHalt{flags, (int)((*q)++ & 1), 0} : MkHalt{d_nohalt, 0, 0}; }
    // mk_<kind>_apply: the argument checks of a device vector that crosses the C ABI, then `enqueue` on the context's stream
    static int apply_standalone(const MkDeviceOp *F, const double *in_dev, double *out_dev);
    void hold() const { users += 1; }
    void release() const {
        if (--users <= 0 && doomed) delete this;
    }
    void destroy() {               // (the mk_*_destroy entry points)
        if (users > 0) doomed = true;
        else delete this;
    }
};

// A Chebyshev object as the device operator it is (mk_cheb.hip): the smoother of every level of mk_amg.hip
const MkDeviceOp *mk_cheb_as_op(const mk_cheb *F);
// A Chebyshev filter as the device operator it is (mk_chebfilt.hip), and what the filtered cycle of mk_trlan.hip asks of it:
// its matrix, its degree, the unwanted interval [a, b] and the reference point a0
struct mk_filter;
constexpr int MK_FILTER_INFO_LEN = 8;
int mk_filter_create(const mk_csr *A, int32_t degree, double a, double b, double a0, mk_filter **out);
void mk_filter_free(mk_filter *F);
const MkDeviceOp *mk_filter_as_op(const mk_filter *F);
void mk_filter_describe(const mk_filter *F, const mk_csr **A, int *degree, double *a, double *b, double *a0);
std::vector<double> mk_filter_table(const mk_filter *F);

// A preconditioner slot.  A solver has two (mk_solver::slot): a square solver uses the first, a least-squares solver both,
// for M (nrows(A) entries) and N (ncols(A) entries).  A diagonal is multiplied inside the loop's kernels (`d`).  With one of
// the general kinds the kernels run with a diagonal of ones (`1.0 * v` is exact) and every preconditioned vector is
// replaced by `apply_slot`'s result right after the kernel that produced it; inner products with it are re-formed by a
// separate stream kernel.
enum MkPreconKind {
    MK_PRECON_NONE = 0,
    MK_PRECON_DIAG,        // mk_solver_set_precon_diag / _lls_precon: the borrowed diagonal is `d` itself
    MK_PRECON_HOST,        // mk_solver_set_precon_callback / _lls_precon_callback: `fn(user, in, out)` on the host, through
                           // pinned buffers
    MK_PRECON_CSR,         // mk_solver_set_precon_csr / _lls_precon_csr: a device matrix or composite `op` (counted in
                           // op->dependents), e.g. the inverted diagonal blocks of block-Jacobi; the product stays in HBM
    MK_PRECON_OBJECT       // the setter pair of a device object's kind, which lives with the kind: a held MkDeviceOp `obj`,
                           // applied by `obj->enqueue` with the loop's halt words and kernel counter
};

struct MkPrecon {
    // what is attached (all that a replacement carries)
    MkPreconKind kind = MK_PRECON_NONE;
    mk_precon_fn fn = nullptr;
    void *user = nullptr;
    const mk_csr *op = nullptr;
    const MkDeviceOp *obj = nullptr;
    const double *d = nullptr;      // what the kernels multiply by: the borrowed diagonal, `ones` for a general kind, or null
    // the slot's own, from the solver's creation to its end
    int64_t len = 0;                // entries of the vectors it takes
    double *ones = nullptr;         // (owned, allocated with the first general kind)
    bool general() const { return kind >= MK_PRECON_HOST; }
    void hold() const;              // take the reference a slot keeps on a device matrix or object
    void release();                 // drop it and go back to MK_PRECON_NONE
    // the replacements the setters hand to mk_set_precon; a null argument gives MK_PRECON_NONE
    static MkPrecon diagonal(const double *diag) {
        MkPrecon p;
        if (diag) p.kind = MK_PRECON_DIAG;
        p.d = diag;
        return p;
    }
    static MkPrecon callback(mk_precon_fn fn, void *user) {
        MkPrecon p;
        if (fn) p.kind = MK_PRECON_HOST;
        p.fn = fn;
        p.user = user;
        return p;
    }
    static MkPrecon matrix(const mk_csr *op) {
        MkPrecon p;
        if (op) p.kind = MK_PRECON_CSR;
        p.op = op;
        return p;
    }
    static MkPrecon object(const MkDeviceOp *obj) {
        MkPrecon p;
        if (obj) p.kind = MK_PRECON_OBJECT;
        p.obj = obj;
        return p;
    }
};

struct mk_solver {
    const mk_csr *A = nullptr;
    const mk_csr *At = nullptr;     // transposed matrix (the least-squares solvers and MK_TRSVD)
    MkPrecon slot[2];               // [0]: a square solver's preconditioner, or M of a least-squares one; [1]: N
    double *h_pin = nullptr, *h_pout = nullptr;   // pinned staging of the host callback, shared by the slots (max of their lengths)
    double *d_ptmp = nullptr;       // product target when a site preconditions a vector in place by a device matrix
    int *d_nohalt = nullptr;        // two zero words: the halt input of a kernel that must run after the loop has ended
    // the square solvers' view of their one slot
    const double *d_prec() const { return slot[0].d; }
    bool general_precon() const { return slot[0].general(); }
    // `next` replaces whatever `into` (one of `slot`) holds; MK_PRECON_NONE leaves it empty.  The messages name the entry
    // point `who`, the slot (`name`: "the preconditioner", "M", "N") and, for an object, what it is (its `noun`).  The one
    // place that validates a replacement, gives a slot its ones and the solver its pinned buffers, and moves a reference.
    int attach(MkPrecon &into, const MkPrecon &next, const char *who, const char *name);
    int apply_precon(const double *in_dev, double *out_dev, bool force = false) {   // out = precon * in ; unless `force`, a no-op once the loop has halted
        return apply_slot(slot[0], in_dev, out_dev, force);
    }
    // out = slot * in for a general kind.  `need_pos` (least squares, beta of lsqr.py:258): a device scalar that must be
    // > 0 for a HOST callback to run, read with the halt word in the one synchronisation; the launches of the device kinds
    // cannot be gated from the host -- their caller gates the product itself (mk_apply_csr_slot) or takes an out-of-place
    // result on the device
    int apply_slot(const MkPrecon &slot, const double *in_dev, double *out_dev, bool force, const double *need_pos = nullptr);
    mk_params prm{};
    int nsigma = 0;                              // MK_MSCG: the shifts of the long parameter block (mk_params_shifts)
    double sigma[MK_MSCG_MAX_SHIFTS] = {};
    int eig_nev = 0, eig_ncv = 0, eig_which = 0, eig_keep = 0;   // MK_TRLAN, MK_LOBPCG, MK_TRSVD: the tail of their long parameter block (mk_params_eig)
    uint64_t eig_seed = 0;
    int ring_cap = 0, ring_cap_setups = 0;       // MK_CG: the tail of mk_params_ring (0: no bound on the ring depth; 0: at every set-up)
    int64_t n = 0;       // local rows = length of every solver vector
    int64_t nx = 0;       // length of vectors that feed an SpMV (n + halo)
    hipStream_t stream = nullptr;

    double *d_scal = nullptr;       // MK_NSCAL
    double *d_part = nullptr;       // MK_NDOT * MK_MAXP
    int *d_halt = nullptr;          // 2
    MkStatus *d_status = nullptr;
    double *d_hist = nullptr;       // 2 * MK_HIST_RING: channel 0 = residual history, channel 1 = solver specific
    MkStatus *h_status = nullptr;   // pinned
    double *h_scal = nullptr;       // pinned, MK_NSCAL
    std::vector<double *> vecs;     // owned device vectors
    std::vector<double *> arena_vecs;   // ... carved from the context's vector arena (mk_arena_reserve): returned, not freed
    std::vector<double> hist;       // drained history (host)
    std::vector<double> hist2;      // second channel (MINRES: direct-error estimates)
    bool use_hist2 = false;
    int64_t hist_drained = 0;

    int64_t q = 0;                  // kernels launched so far (halt parity)
    int64_t it = 0;                 // loop passes enqueued so far
    bool is_setup = false, halted = false;
    bool counted_user = false;      // this solver is in its matrix's solver_users count (mk_csr_march_pref)
    int np_spmv = 1, np_stream = 1; // partial counts consumers must add up

    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_iterate_ms = 0.0;
    std::vector<hipEvent_t> spmv_ev;    // pairs
    int64_t spmv_timed = 0;
    double spmv_ms = 0.0;
    int spmv_sample_stride = 0;         // 0 = no per-kernel events

    virtual ~mk_solver();
    virtual int setup(const double *rhs, const double *guess) = 0;
    virtual int enqueue_pass() = 0;                 // one pass of the reference loop body
    virtual int finish(mk_result *res) = 0;
    virtual const double *x() const = 0;
    virtual const double *vector(int) const { return nullptr; }
    virtual int64_t vector_len(int) const { return n; }   // entries of `vector(i)` (multi-shift CG's record is not a solver vector)
    virtual bool takes_precon() const { return false; }
    // the tail of mk_params_filter: a Chebyshev filter as the spectral transformation of the loop (MK_TRLAN only)
    virtual int make_filter(int32_t, double, double, double) {
        return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_create: this solver kind takes no spectral transformation (the block "
                       "mk_params_filter is thick-restart Lanczos', MK_TRLAN)");
    }
    virtual bool is_fused() const { return false; }   // CG on a format-9 matrix: the x / p update rides in the next product kernel
    // work a loop defers beyond its passes (CG: the x update over a ring of directions): `drain` enqueues what is applicable at
    // the end of an iterate call, inside its timed region; `unapplied` counts completed passes whose update is still missing
    virtual int drain() { return MK_OK; }
    virtual int64_t unapplied() const { return 0; }
    // enqueue only the solver's (fused) SpMV kernel, exactly as a loop pass launches it; used to time
    // that kernel back to back.  Overwrites the product vector and its partial sums.
    // `which`: 0 = the first product of a pass, 1 = the second (BiCGSTAB / CGS / TFQMR: the product on z; least squares:
    // the A' u product with its fused v update); run without its gate.
    virtual int enqueue_spmv_only(int which = 0) { return mk_fail(MK_ERR_UNSUPPORTED, "SpMV timing is not wired for this solver"); }

    int init_common(const mk_csr *A_, const mk_params *p);
    int alloc_vec(double **out, int64_t len);
    MkHalt next_halt() { return MkHalt{d_halt, (int)(q++ & 1), mk_comm_active() ? MK_MAXP : 0}; }
    int poll();                                     // status + scalars + history -> host
    int iterate(int64_t max_iters, int64_t *done);
    int allreduce(int slot0, int nslots);           // partial sums across ranks (multi-GPU only)
    int exchange(double *x_ext);                    // halo / allgather before an SpMV
    void fill_result(mk_result *res) const;
    // SpMV timing helpers
    void spmv_begin();
    void spmv_end();
    int collect_spmv_timing();
};

// Where every extern "C" setter ends: `next` into the slot of a square solver (`side` < 0; refused if the solver kind has no
// hook) or into side M / N of a least-squares solver (refused on any other); then mk_solver::attach
int mk_set_precon(mk_solver *s, int side, const MkPrecon &next, const char *who);

mk_solver *mk_make_cg();
mk_solver *mk_make_bicgstab();
mk_solver *mk_make_cgs();
mk_solver *mk_make_tfqmr();
mk_solver *mk_make_minres();
mk_solver *mk_make_symmlq();
mk_solver *mk_make_lls(int kind);
mk_solver *mk_make_gmres();
mk_solver *mk_make_idr();
mk_solver *mk_make_pcg();
mk_solver *mk_make_mscg();
mk_solver *mk_make_trlan();
mk_solver *mk_make_lobpcg();
mk_solver *mk_make_trsvd();

#ifdef __HIPCC__
// ------------------------------------------------------------------ small shared kernels
struct MkOpNegCopy {            // out = -in                    (cg.py:85,104)
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *in;
    double *out;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 v = mk_ld2(in, i);
        v.x = -v.x;
        v.y = -v.y;
        mk_st2(out, i, v);
    }
    __device__ void one(int64_t i, double *) { out[i] = -in[i]; }
};

struct MkOpCopy {               // out = in
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *in;
    double *out;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) { mk_st2(out, i, mk_ld2(in, i)); }
    __device__ void one(int64_t i, double *) { out[i] = in[i]; }
};

template <int SIGN>             // y = y + SIGN * x   (exact add/sub, no multiply)
struct MkOpAddTo {
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *x;
    double *y;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 a = mk_ld2(x, i), b = mk_ld2(y, i);
        b.x = SIGN > 0 ? b.x + a.x : b.x - a.x;
        b.y = SIGN > 0 ? b.y + a.y : b.y - a.y;
        mk_st2(y, i, b);
    }
    __device__ void one(int64_t i, double *) { y[i] = SIGN > 0 ? y[i] + x[i] : y[i] - x[i]; }
};

struct MkOpSub {                // out = a - b
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *a, *b;
    double *out;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 u = mk_ld2(a, i), v = mk_ld2(b, i);
        u.x -= v.x;
        u.y -= v.y;
        mk_st2(out, i, u);
    }
    __device__ void one(int64_t i, double *) { out[i] = a[i] - b[i]; }
};

struct MkOpMul {                // out = a * b elementwise  (DiagonalOperator matvec `diag*x`, linop.py:503)
    static constexpr int NACC = 0, SLOT0 = 0;
    const double *a, *b;
    double *out;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *) {
        double2 u = mk_ld2(a, i), v = mk_ld2(b, i);
        u.x *= v.x;
        u.y *= v.y;
        mk_st2(out, i, u);
    }
    __device__ void one(int64_t i, double *) { out[i] = a[i] * b[i]; }
};

template <int SLOT>             // partial sums of dot(a, b) into slot SLOT
struct MkOpDot {
    static constexpr int NACC = 1, SLOT0 = SLOT;
    const double *a, *b;
    __device__ bool prologue(double *, bool) { return false; }
    __device__ bool skip() const { return false; }
    __device__ void pair(int64_t i, double *acc) {
        double2 u = mk_ld2(a, i), v = mk_ld2(b, i);
        acc[0] += u.x * v.x;
        acc[0] += u.y * v.y;
    }
    __device__ void one(int64_t i, double *acc) { acc[0] += a[i] * b[i]; }
};

// Product vectors of problems beyond the Infinity Cache are written once and read by the NEXT kernel from HBM: storing them
// non-temporally keeps them from pushing the x windows out of the L2 (mk_store_nt, mk_device.h: -5 ... -7 % on the CG product
// at 512^3).  CG carries the choice as a template parameter; the other loops' epilogues take it at run time through this
// helper -- an inline-asm store in the `nt` branch, because the compiler merges `if (nt) nontemporal_store else store` into
// ONE plain store (round 3's finding) -- so that no kernel is instantiated twice for it.  `nt` is launch uniform.
__device__ __forceinline__ void mk_store_stream(double *p, double v, int nt) {
    if (nt) asm volatile("global_store_dwordx2 %0, %1, off nt" : : "v"(p), "v"(v) : "memory");
    else *p = v;
}

struct MkPlainEpi {             // y = A x, nothing fused
    static constexpr int NACC = 0, SLOT0 = 0;
    static constexpr bool SYM_MARCH = true;                  // (may meet format 11: mk_device.h MkSymMarch)
    double *y;
    __device__ void prologue(double *) {}
    __device__ double xin(double v) const { return v; }
    __device__ void row(int64_t r, double s, double *) { y[r] = s; }
    // the brick march on a general geometry (mk_spmv_fmt9.h, GEN): rows r, r + 1 where they exist
    __device__ void row2_m(int64_t r, mk_d2 s, mk_d2, bool oka, bool okb, double *dump, double *) {
        *reinterpret_cast<mk_d2u *>(okb ? y + r : dump) = s;
        if (oka && !okb) y[r] = s.x;
    }
};

template <class Op>
static inline int mk_launch_stream(mk_solver *s, const Op &op, int64_t n) {
    const int grid = mk_grid_stream(n);
    hipLaunchKernelGGL(mk_stream_kernel<Op>, dim3(grid), dim3(MK_BLOCK), 0, s->stream, op, n, s->next_halt(),
                       s->d_part);
    return MK_OK;
}

template <class Epi, class Gate = MkNoGate>
static inline int mk_launch_spmv_on(mk_solver *s, const mk_csr *M, const double *x, const Epi &epi,
                                    const Gate &gate = Gate()) {
    mk_spmv_launch_blocks(M, mk_grid_spmv_for(M), s->stream, x, epi, gate, [&] { return s->next_halt(); }, s->d_part);
    return MK_OK;
}

// out = op * in by the device matrix of a preconditioner slot (mk_solver::apply_slot's MK_PRECON_CSR case).  Like every kernel
// of the loop the product obeys the halt words: once the loop condition has failed it is a no-op, exactly when the reference
// applies nothing more -- unless `force` (set-up).  `gate` is MkNoGate for every site but N of the least-squares loops,
// whose product runs under the A' product's own gate (mk_lls.hip, GateV).
template <class Gate>
static inline int mk_apply_csr_slot(mk_solver *s, const MkPrecon &slot, const double *in_dev, double *out_dev, bool force,
                                    const Gate &gate) {
    const mk_csr *op = slot.op;
    const int64_t len = slot.len;
    double *dst = (in_dev == out_dev) ? s->d_ptmp : out_dev;
    const int grid = mk_grid_spmv_for(op);
    if (force) {
        mk_spmv_launch_blocks(op, grid, s->stream, in_dev, MkPlainEpi{dst}, gate,
                              [&] { return MkHalt{s->d_nohalt, 0, 0}; }, s->d_part);
        if (dst != out_dev) MK_HIP(hipMemcpyAsync(out_dev, dst, sizeof(double) * (size_t)len, hipMemcpyDeviceToDevice, s->stream));
    } else {
        mk_spmv_launch_blocks(op, grid, s->stream, in_dev, MkPlainEpi{dst}, gate, [&] { return s->next_halt(); }, s->d_part);
        if (dst != out_dev) mk_launch_stream(s, MkOpCopy{dst, out_dev}, len);
    }
    return mk_ctx().pending_rc;
}

template <class Epi, class Gate = MkNoGate>
static inline int mk_launch_spmv(mk_solver *s, const double *x, const Epi &epi, bool timed = true,
                                 const Gate &gate = Gate()) {
    const mk_csr *A = s->A;
    if (timed) s->spmv_begin();
    const MkPlan *plan = A->ex.pending ? mk_csr_plan(A) : nullptr;
    const bool march = plan && mk_fmt_march(plan->fmt);
    int za, zb;
    const bool thin = MkSymMarch<Epi>::value;   // (mk_pen_split: only the first and the last plane wait)
    if (A->ex.pending && march && (!mk_march_kernel_for<Epi>(plan) || !mk_pen_split(plan, &za, &zb, thin))) {
        // a slab of too few planes to split -- or a loop without a kernel for this march format, whose product runs as the
        // CSR gather kernel over ALL rows (a plane range means nothing to it): the messages first, then one launch
        int rc = mk_exchange_wait(A, s->stream);
        if (rc != MK_OK) return rc;
        mk_spmv_launch_blocks(A, mk_grid_spmv_for(A), s->stream, x, epi, gate, [&] { return s->next_halt(); }, s->d_part);
    } else if (A->ex.pending) {
        // halo exchange in flight: rows that need no received entry first, the others once the messages are in
        // (the two launches write disjoint ranges of the partial-sum slots)
        int g1, g2;
        const MkCsrView v1 = mk_view_part(A, 1, 0, thin);
        if (march) {                                         // plane ranges of the brick march (mk_pen_split)
            g1 = mk_pen_items(v1);
            g2 = mk_pen_items(mk_view_part(A, 2, 0, thin));
            // (the kernels stride their items by the grid: a plane of >= 1024 bricks must not leave the interior launch a
            //  grid of 0 -- at most half of the partial-sum slots for the boundary planes)
            if (g2 > MK_MAXP / 2) g2 = MK_MAXP / 2;
            if (g1 + g2 > MK_MAXP) g1 = MK_MAXP - g2;
        } else {
            mk_grid_spmv_parts(A, A->ex.n_int, A->ex.n_bnd, &g1, &g2);
        }
        mk_spmv_launch_view(v1, g1, s->stream, x, epi, gate, s->next_halt(), s->d_part);
        int rc = mk_exchange_wait(A, s->stream);
        if (rc != MK_OK) return rc;
        mk_spmv_launch_view(mk_view_part(A, 2, g1, thin), g2, s->stream, x, epi, gate, s->next_halt(), s->d_part);
    } else {
        mk_spmv_launch_blocks(A, mk_grid_spmv_for(A), s->stream, x, epi, gate, [&] { return s->next_halt(); }, s->d_part);
    }
    if (timed) s->spmv_end();
    return MK_OK;
}
#endif
