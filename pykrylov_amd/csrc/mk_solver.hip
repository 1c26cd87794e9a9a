// mk_solver.hip -- generic driver of the device-resident solver loops + C ABI dispatch.
#include "mk_solver.h"

#include <algorithm>
#include <cmath>

int mk_solver::init_common(const mk_csr *A_, const mk_params *p) {
    A = A_;
    A->dependents += 1;              // (borrowed for the solver's lifetime: destroying A meanwhile is deferred)
    prm = *p;
    n = A->ex.mode >= 0 ? A->ex.n_local : A->nrows;
    const bool lls = prm.kind >= MK_LSQR && prm.kind <= MK_CRAIGMR;
    const bool rectangular_ok = lls || prm.kind == MK_TRSVD;
    slot[0].len = n;
    slot[1].len = lls ? A->ncols : 0;
    if (lls && A->ex.mode >= 0)
        return mk_fail(MK_ERR_UNSUPPORTED, "the least-squares solvers partition by row blocks with a replicated column "
                       "space (mk_csr_set_row_block), not with a halo / all-gather exchange plan");
    if (!rectangular_ok && A->ex.mode < 0 && A->nrows != A->ncols)
        return mk_fail(MK_ERR_ARG, "solver needs a square operator, got %lld x %lld", (long long)A->nrows,
                       (long long)A->ncols);
    nx = A->x_len();
    stream = mk_ctx().stream;
    MK_HIP(hipMalloc((void **)&d_scal, sizeof(double) * MK_NSCAL));
    MK_HIP(hipMalloc((void **)&d_part, sizeof(double) * MK_NDOT * MK_MAXP));
    MK_HIP(hipMalloc((void **)&d_halt, 2 * sizeof(int)));
    MK_HIP(hipMalloc((void **)&d_nohalt, 2 * sizeof(int)));
    MK_HIP(hipMemsetAsync(d_nohalt, 0, 2 * sizeof(int), stream));
    MK_HIP(hipMalloc((void **)&d_status, sizeof(MkStatus)));
    MK_HIP(hipMalloc((void **)&d_hist, sizeof(double) * 2 * MK_HIST_RING));
    MK_HIP(hipHostMalloc((void **)&h_status, sizeof(MkStatus), hipHostMallocDefault));
    MK_HIP(hipHostMalloc((void **)&h_scal, sizeof(double) * MK_NSCAL, hipHostMallocDefault));
    MK_HIP(hipEventCreate(&ev0));
    MK_HIP(hipEventCreate(&ev1));
    // with several ranks every consumer adds all MK_MAXP slots (unused ones stay zero) so that the
    // all-reduced partial vectors mean the same thing on every rank
    const bool multi = mk_comm_active() != 0;
    np_spmv = multi ? MK_MAXP : mk_grid_spmv_for(A);
    np_stream = multi ? MK_MAXP : mk_grid_stream(n);
    spmv_sample_stride = prm.spmv_event_stride;
    return MK_OK;
}

int mk_solver::apply_slot(const MkPrecon &slot, const double *in_dev, double *out_dev, bool force, const double *need_pos) {
    const int64_t len = slot.len;
    switch (slot.kind) {
        case MK_PRECON_OBJECT: {
            // out = P in by the object's own launches (the factor's sweeps, the chain of the two-loop recursion); each obeys
            // the halt words like the product below
            const int rc = force ? slot.obj->enqueue(in_dev, out_dev, stream, nullptr, nullptr)
                                 : slot.obj->enqueue(in_dev, out_dev, stream, d_halt, &q);
            return rc != MK_OK ? rc : mk_ctx().pending_rc;
        }
        case MK_PRECON_CSR:                                  // out = op * in on the device
            return mk_apply_csr_slot(this, slot, in_dev, out_dev, force, MkNoGate());
        case MK_PRECON_HOST: {
            int h = 0;
            double pos = 1.0;
            MK_HIP(hipMemcpyAsync(&h, d_halt + (q & 1), sizeof(int), hipMemcpyDeviceToHost, stream));   // the next kernel's word
            if (need_pos) MK_HIP(hipMemcpyAsync(&pos, need_pos, sizeof(double), hipMemcpyDeviceToHost, stream));
            if (len > 0) MK_HIP(hipMemcpyAsync(h_pin, in_dev, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost, stream));
            MK_HIP(hipStreamSynchronize(stream));
            if (h && !force) return MK_OK;                   // the loop has ended: the reference applies nothing more
            if (!(pos > 0)) return MK_OK;                    // ... or does not reach this site (lsqr.py:258)
            if (slot.fn(slot.user, h_pin, h_pout) != 0) {
                const int rc = mk_fail(MK_ERR_STATE, "the host preconditioner callback reported a failure");
                if (mk_ctx().pending_rc == MK_OK) mk_ctx().pending_rc = rc;
                return rc;
            }
            if (len > 0) MK_HIP(hipMemcpyAsync(out_dev, h_pout, sizeof(double) * (size_t)len, hipMemcpyHostToDevice, stream));
            return MK_OK;
        }
        default: return MK_OK;                               // (a diagonal acts inside the kernels)
    }
}

void MkPrecon::hold() const {
    if (kind == MK_PRECON_CSR) op->dependents += 1;
    if (kind == MK_PRECON_OBJECT) obj->hold();
}

void MkPrecon::release() {
    if (kind == MK_PRECON_CSR) mk_release_operand(op);
    if (kind == MK_PRECON_OBJECT) obj->release();
    kind = MK_PRECON_NONE;
    fn = nullptr;
    user = nullptr;
    op = nullptr;
    obj = nullptr;
    d = nullptr;
}

mk_solver::~mk_solver() {
    if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);   // (an object released below may free its memory)
    for (MkPrecon &p : slot) {
        p.release();
        hipFree(p.ones);
    }
    if (At) mk_release_operand(At);
    if (A && counted_user) mk_csr_count_users(A, -1);
    if (A) mk_release_operand(A);
    hipFree(d_ptmp);
    hipFree(d_nohalt);
    if (h_pin) hipHostFree(h_pin);
    if (h_pout) hipHostFree(h_pout);
    if (mk_ctx().ready) hipStreamSynchronize(mk_ctx().stream);
    for (double *v : vecs) hipFree(v);
    if (!arena_vecs.empty()) {                               // the arena is reusable once its last vector is back
        MkContext &c = mk_ctx();
        c.arena_live -= (int)arena_vecs.size();
        if (c.arena_live <= 0) {
            c.arena_live = 0;
            c.arena_off = 0;
        }
    }
    for (hipEvent_t e : spmv_ev) hipEventDestroy(e);
    hipFree(d_scal);
    hipFree(d_part);
    hipFree(d_halt);
    hipFree(d_status);
    hipFree(d_hist);
    if (h_status) hipHostFree(h_status);
    if (h_scal) hipHostFree(h_scal);
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
}

int mk_solver::alloc_vec(double **out, int64_t len) {
    double *p = nullptr;
    const size_t bytes = sizeof(double) * (size_t)(len > 0 ? len : 1) + 16;
    MkContext &c = mk_ctx();
    const size_t step = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);   // 2 MiB granules
    if (c.arena && c.arena_off + step <= c.arena_size) {     // carved from the arena reserved before the matrix
        p = reinterpret_cast<double *>(c.arena + c.arena_off);
        c.arena_off += step;
        c.arena_live += 1;
        arena_vecs.push_back(p);
    } else {
        MK_HIP(hipMalloc((void **)&p, bytes));
        vecs.push_back(p);
    }
    MK_HIP(hipMemsetAsync(p, 0, bytes, stream));
    *out = p;
    return MK_OK;
}

extern "C" int mk_arena_reserve(size_t bytes) {
    MK_REQUIRE_INIT();
    MkContext &c = mk_ctx();
    if (c.arena_live > 0) return mk_fail(MK_ERR_STATE, "mk_arena_reserve: %d vectors of the current arena are still in use", c.arena_live);
    if (c.arena) {
        MK_HIP(hipStreamSynchronize(c.stream));
        MK_HIP(hipFree(c.arena));
        c.arena = nullptr;
        c.arena_size = c.arena_off = 0;
    }
    if (bytes == 0) return MK_OK;
    MK_HIP(hipMalloc((void **)&c.arena, bytes));
    c.arena_size = bytes;
    c.arena_off = 0;
    return MK_OK;
}

int mk_solver::allreduce(int slot0, int nslots) {
    if (!mk_comm_active()) return MK_OK;
    return mk_comm_allreduce_sum(d_part + (size_t)slot0 * MK_MAXP, (int64_t)nslots * MK_MAXP, stream);
}

int mk_solver::exchange(double *x_ext) {
    if (A->ex.mode < 0) return MK_OK;
    return mk_exchange_begin(A, x_ext);                    // mk_launch_spmv completes it
}

void mk_solver::spmv_begin() {
    if (spmv_sample_stride <= 0 || (it % spmv_sample_stride) != 0) return;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    spmv_ev.push_back(a);
    spmv_ev.push_back(b);
    hipEventRecord(a, stream);
}

void mk_solver::spmv_end() {
    if (spmv_sample_stride <= 0 || (it % spmv_sample_stride) != 0 || spmv_ev.empty()) return;
    hipEventRecord(spmv_ev.back(), stream);
}

int mk_solver::collect_spmv_timing() {
    for (size_t i = 0; i + 1 < spmv_ev.size(); i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, spmv_ev[i], spmv_ev[i + 1]) == hipSuccess) {
            spmv_ms += ms;
            spmv_timed += 1;
        }
        hipEventDestroy(spmv_ev[i]);
        hipEventDestroy(spmv_ev[i + 1]);
    }
    spmv_ev.clear();
    return MK_OK;
}

int mk_solver::poll() {
    MK_HIP(hipMemcpyAsync(h_status, d_status, sizeof(MkStatus), hipMemcpyDeviceToHost, stream));
    MK_HIP(hipMemcpyAsync(h_scal, d_scal, sizeof(double) * MK_NSCAL, hipMemcpyDeviceToHost, stream));
    int h[2];
    MK_HIP(hipMemcpyAsync(h, d_halt, sizeof(h), hipMemcpyDeviceToHost, stream));
    MK_HIP(hipStreamSynchronize(stream));
    halted = h[q & 1] != 0;      // the word the NEXT kernel would read
    // drain new residual-history entries from the ring
    const int64_t have = h_status->hist_len;
    if (have > hist_drained) {
        if (have - hist_drained > MK_HIST_RING)
            return mk_fail(MK_ERR_STATE, "history ring overrun (%lld new entries)", (long long)(have - hist_drained));
        hist.resize((size_t)have);
        if (use_hist2) hist2.resize((size_t)have);
        int64_t pos = hist_drained;
        while (pos < have) {
            const int64_t off = pos % MK_HIST_RING;
            int64_t cnt = have - pos;
            if (cnt > MK_HIST_RING - off) cnt = MK_HIST_RING - off;
            MK_HIP(hipMemcpyAsync(hist.data() + pos, d_hist + off, sizeof(double) * (size_t)cnt,
                                  hipMemcpyDeviceToHost, stream));
            if (use_hist2)
                MK_HIP(hipMemcpyAsync(hist2.data() + pos, d_hist + MK_HIST_RING + off, sizeof(double) * (size_t)cnt,
                                      hipMemcpyDeviceToHost, stream));
            pos += cnt;
        }
        MK_HIP(hipStreamSynchronize(stream));
        hist_drained = have;
    }
    return MK_OK;
}

int mk_solver::iterate(int64_t max_iters, int64_t *done) {
    if (!is_setup) return mk_fail(MK_ERR_STATE, "mk_solver_iterate before mk_solver_setup");
    int64_t launched = 0;
    int64_t batch = 16;
    const int64_t itn0 = h_status->itn;
    MK_HIP(hipEventRecord(ev0, stream));
    while (!halted && launched < max_iters) {
        int64_t todo = max_iters - launched;
        if (todo > batch) todo = batch;
        for (int64_t k = 0; k < todo; ++k) {
            int rc = enqueue_pass();
            // a host operator / preconditioner callback failed inside this pass: stop enqueueing at once -- the
            // caller's operator must not be called again on vectors that no longer mean anything
            if (rc == MK_OK && mk_ctx().pending_rc != MK_OK) rc = mk_ctx().pending_rc;
            if (rc != MK_OK) {
                mk_ctx().pending_rc = MK_OK;                 // (reported here: must not resurface in a later call)
                return rc;
            }
            ++it;
        }
        MK_HIP(hipGetLastError());
        if (mk_ctx().pending_rc != MK_OK) {                  // (a host operator callback failed)
            const int prc = mk_ctx().pending_rc;
            mk_ctx().pending_rc = MK_OK;
            return prc;
        }
        launched += todo;
        int rc = poll();
        if (rc != MK_OK) return rc;
        if (batch < MK_BATCH_MAX) batch *= 2;
    }
    {   // what the passes of this call deferred runs inside the call, before its closing event
        const int rc = drain();
        if (rc != MK_OK) return rc;
    }
    MK_HIP(hipEventRecord(ev1, stream));
    MK_HIP(hipEventSynchronize(ev1));
    float ms = 0.f;
    MK_HIP(hipEventElapsedTime(&ms, ev0, ev1));
    last_iterate_ms = ms;
    collect_spmv_timing();
    if (done) *done = h_status->itn - itn0;
    return MK_OK;
}

void mk_solver::fill_result(mk_result *res) const {
    memset(res, 0, sizeof(*res));
    res->struct_size = (int32_t)sizeof(mk_result);
    res->halted = halted ? 1 : 0;
    res->nMatvec = h_status->nMatvec;
    res->itn = h_status->itn;
    res->hist_len = (int64_t)hist.size();
    res->converged = h_status->converged;
    res->definite = h_status->definite;
    res->istop = h_status->istop;
}

// ======================================================================================
// C ABI
// ======================================================================================
extern "C" int mk_solver_create(const mk_csr *A, const mk_params *params, mk_solver **out) {
    MK_REQUIRE_INIT();
    MK_ARG(A && params && out);
    // the short block, or a long one whose tail carries the shifts of MK_MSCG or the eigenproblem of MK_TRLAN / MK_LOBPCG / MK_TRSVD (every kind
    // takes any of them)
    const mk_params_shifts *shifts = nullptr;
    const mk_params_eig *eig = nullptr;
    const mk_params_filter *filt = nullptr;                  // ... or, behind the eigenproblem, the Chebyshev filter of MK_TRLAN
    const mk_params_ring *ringp = nullptr;                   // ... or a bound on the depth of MK_CG's ring of directions
    if (params->struct_size == (int32_t)sizeof(mk_params_filter)) {
        filt = reinterpret_cast<const mk_params_filter *>(params);
        eig = &filt->eig;
    } else if (params->struct_size == (int32_t)sizeof(mk_params_shifts)) shifts = reinterpret_cast<const mk_params_shifts *>(params);
    else if (params->struct_size == (int32_t)sizeof(mk_params_eig)) eig = reinterpret_cast<const mk_params_eig *>(params);
    else if (params->struct_size == (int32_t)sizeof(mk_params_ring)) ringp = reinterpret_cast<const mk_params_ring *>(params);
    else MK_ARG(params->struct_size == (int32_t)sizeof(mk_params));
    if (ringp && (ringp->xdefer_cap < 0 || ringp->xdefer_cap > 32 || ringp->xdefer_cap_setups < 0))
        return mk_fail(MK_ERR_ARG, "mk_solver_create: xdefer_cap = %d, must be 0 (no bound) .. 32, for xdefer_cap_setups = %d >= 0 "
                       "set-ups (0: all)", (int)ringp->xdefer_cap, (int)ringp->xdefer_cap_setups);
    mk_solver *s = nullptr;
    switch (params->kind) {
        case MK_CG: s = mk_make_cg(); break;
        case MK_BICGSTAB: s = mk_make_bicgstab(); break;
        case MK_CGS: s = mk_make_cgs(); break;
        case MK_TFQMR: s = mk_make_tfqmr(); break;
        case MK_MINRES: s = mk_make_minres(); break;
        case MK_SYMMLQ: s = mk_make_symmlq(); break;
        case MK_LSQR:
        case MK_LSMR:
        case MK_CRAIG:
        case MK_CRAIGMR: s = mk_make_lls(params->kind); break;
        case MK_GMRES:
            if (params->restart < 1 || params->restart > MK_GMRES_MAX_RESTART)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: GMRES restart = %d, must be 1 .. %d", (int)params->restart,
                               MK_GMRES_MAX_RESTART);
            if (A->ex.mode >= 0 || A->row_block)
                return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_create: the operator is row-partitioned (it carries an exchange "
                               "plan or a row block); GMRES is single-GPU");
            s = mk_make_gmres();
            break;
        case MK_IDR:
            if (A->ex.mode >= 0 || A->row_block)
                return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_create: the operator is row-partitioned (it carries an exchange "
                               "plan or a row block); IDR is single-GPU");
            s = mk_make_idr();
            break;
        case MK_PCG:
            if (A->ex.mode >= 0 || A->row_block)
                return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_create: the operator is row-partitioned (it carries an exchange "
                               "plan or a row block); PCG is single-GPU");
            s = mk_make_pcg();
            break;
        case MK_MSCG:
            if (!shifts)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: multi-shift CG takes its shifts in the long parameter block "
                               "(struct_size = sizeof(mk_params_shifts))");
            if (shifts->nsigma < 1 || shifts->nsigma > MK_MSCG_MAX_SHIFTS)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: multi-shift CG nsigma = %d, must be 1 .. %d", (int)shifts->nsigma,
                               MK_MSCG_MAX_SHIFTS);
            for (int k = 0; k < shifts->nsigma; ++k)
                if (!std::isfinite(shifts->sigma[k]))
                    return mk_fail(MK_ERR_ARG, "mk_solver_create: multi-shift CG sigma[%d] is not finite", k);
            if (A->ex.mode >= 0 || A->row_block)
                return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_create: the operator is row-partitioned (it carries an exchange "
                               "plan or a row block); multi-shift CG is single-GPU");
            s = mk_make_mscg();
            break;
        case MK_TRLAN: {
            if (!eig)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: thick-restart Lanczos takes nev, ncv, which, keep and seed in its "
                               "long parameter block (struct_size = sizeof(mk_params_eig))");
            if (A->ex.mode >= 0 || A->row_block)
                return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_create: the operator is row-partitioned (it carries an exchange "
                               "plan or a row block); thick-restart Lanczos is single-GPU");
            const int64_t top = A->nrows < MK_TRLAN_MAX_NCV ? A->nrows : MK_TRLAN_MAX_NCV;
            if (!(1 <= eig->nev && eig->nev < eig->ncv && (int64_t)eig->ncv <= top))
                return mk_fail(MK_ERR_ARG, "mk_solver_create: thick-restart Lanczos nev = %d, ncv = %d, must be 1 <= nev < ncv <= "
                               "min(n, %d) = %lld", (int)eig->nev, (int)eig->ncv, MK_TRLAN_MAX_NCV, (long long)top);
            if (eig->keep != 0 && !(eig->nev <= eig->keep && eig->keep < eig->ncv))
                return mk_fail(MK_ERR_ARG, "mk_solver_create: thick-restart Lanczos keep = %d, must be 0 (automatic) or nev = %d "
                               "<= keep < ncv = %d", (int)eig->keep, (int)eig->nev, (int)eig->ncv);
            if (eig->which != 0 && eig->which != 1)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: thick-restart Lanczos which = %d, must be 0 (smallest) or 1 "
                               "(largest)", (int)eig->which);
            s = mk_make_trlan();
            s->eig_nev = eig->nev;
            s->eig_ncv = eig->ncv;
            s->eig_which = eig->which;
            s->eig_keep = eig->keep ? eig->keep : std::min(eig->nev + (eig->ncv - eig->nev) / 2, eig->ncv - 1);
            s->eig_seed = eig->seed;
            break;
        }
        case MK_LOBPCG: {
            if (!eig)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: LOBPCG takes nev, the block size (in ncv), which and seed in its long "
                               "parameter block (struct_size = sizeof(mk_params_eig))");
            if (A->ex.mode >= 0 || A->row_block)
                return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_create: the operator is row-partitioned (it carries an exchange "
                               "plan or a row block); LOBPCG is single-GPU");
            if (params->restart != 0) {                      // the probe of the Gram kernel (a test hook: mikrylov.h)
                if (params->restart != 1 || !(1 <= eig->ncv && eig->ncv <= 3 * MK_LOBPCG_MAX_BLOCK))
                    return mk_fail(MK_ERR_ARG, "mk_solver_create: LOBPCG's Gram probe takes restart = 1 and 1 <= ncv <= %d columns",
                                   3 * MK_LOBPCG_MAX_BLOCK);
            } else {
                const int64_t top = A->nrows / 3 < MK_LOBPCG_MAX_BLOCK ? A->nrows / 3 : MK_LOBPCG_MAX_BLOCK;
                if (!(1 <= eig->nev && eig->nev <= eig->ncv && (int64_t)eig->ncv <= top))
                    return mk_fail(MK_ERR_ARG, "mk_solver_create: LOBPCG nev = %d, block = %d, must be 1 <= nev <= block <= "
                                   "min(%d, n / 3) = %lld", (int)eig->nev, (int)eig->ncv, MK_LOBPCG_MAX_BLOCK, (long long)top);
            }
            if (eig->keep != 0)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: LOBPCG keep = %d, must be 0", (int)eig->keep);
            if (eig->which != 0 && eig->which != 1)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: LOBPCG which = %d, must be 0 (smallest) or 1 (largest)",
                               (int)eig->which);
            s = mk_make_lobpcg();
            s->eig_nev = eig->nev;
            s->eig_ncv = eig->ncv;
            s->eig_which = eig->which;
            s->eig_seed = eig->seed;
            break;
        }
        case MK_TRSVD: {
            if (!eig)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: the thick-restart SVD takes nev (the triplets wanted), ncv, which, "
                               "keep and seed in its long parameter block (struct_size = sizeof(mk_params_eig))");
            if (A->ex.mode >= 0 || A->row_block)
                return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_create: the operator is row-partitioned (it carries an exchange "
                               "plan or a row block); the thick-restart SVD is single-GPU");
            if (A->nrows < A->ncols)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: the thick-restart SVD takes a tall operator (nrows >= ncols), got "
                               "%lld x %lld; hand it the transpose and swap the left and right vectors", (long long)A->nrows,
                               (long long)A->ncols);
            const int64_t top = A->ncols < MK_TRLAN_MAX_NCV ? A->ncols : MK_TRLAN_MAX_NCV;
            if (!(1 <= eig->nev && eig->nev < eig->ncv && (int64_t)eig->ncv <= top))
                return mk_fail(MK_ERR_ARG, "mk_solver_create: thick-restart SVD nev = %d, ncv = %d, must be 1 <= nev < ncv <= "
                               "min(ncols, %d) = %lld", (int)eig->nev, (int)eig->ncv, MK_TRLAN_MAX_NCV, (long long)top);
            if (eig->keep != 0 && !(eig->nev <= eig->keep && eig->keep < eig->ncv))
                return mk_fail(MK_ERR_ARG, "mk_solver_create: thick-restart SVD keep = %d, must be 0 (automatic) or nev = %d "
                               "<= keep < ncv = %d", (int)eig->keep, (int)eig->nev, (int)eig->ncv);
            if (eig->which != 0 && eig->which != 1)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: thick-restart SVD which = %d, must be 0 (smallest) or 1 "
                               "(largest)", (int)eig->which);
            if (params->reorth != 0 && params->reorth != 1)
                return mk_fail(MK_ERR_ARG, "mk_solver_create: thick-restart SVD reorth = %d, must be 1 (both bases) or 0 (the "
                               "V basis only)", (int)params->reorth);
            s = mk_make_trsvd();
            s->eig_nev = eig->nev;
            s->eig_ncv = eig->ncv;
            s->eig_which = eig->which;
            s->eig_keep = eig->keep ? eig->keep : std::min(eig->nev + (eig->ncv - eig->nev) / 2, eig->ncv - 1);
            s->eig_seed = eig->seed;
            break;
        }
        default: break;
    }
    if (!s) return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_create: solver kind %d is not available", params->kind);
    // (before the partial-sum counts are sized for the format in use; PCG's and multi-shift CG's product kernels are CG's,
    //  mk_cg_epi.h)
    // (the probe of a Chebyshev filter is no loop on A: it neither states a preference nor counts as a user, so a CG solver's
    //  format-11 matrix keeps its format and the filter's steps take the gather kernel on it, mk_chebfilt.hip)
    const bool probe = filt && params->kind == MK_TRLAN && params->restart == 1;
    if (!probe) mk_csr_march_pref(A, params->kind == MK_CG || params->kind == MK_PCG || params->kind == MK_MSCG ? 1 : 0);
    if (shifts && params->kind == MK_MSCG) {
        s->nsigma = shifts->nsigma;
        memcpy(s->sigma, shifts->sigma, sizeof(double) * (size_t)shifts->nsigma);
    }
    if (ringp && params->kind == MK_CG) {
        s->ring_cap = ringp->xdefer_cap;
        s->ring_cap_setups = ringp->xdefer_cap_setups;
    }
    int rc = s->init_common(A, params);
    if (rc != MK_OK) {
        delete s;
        return rc;
    }
    if (!probe) {
        mk_csr_count_users(A, 1);
        s->counted_user = true;
    }
    if (filt && (rc = s->make_filter(filt->degree, filt->a, filt->b, filt->a0)) != MK_OK) {
        delete s;
        return rc;
    }
    *out = s;
    return MK_OK;
}

extern "C" int mk_solver_set_transpose(mk_solver *s, const mk_csr *At) {
    MK_ARG(s && At);
    MK_ARG(At->nrows == s->A->ncols && At->ncols == s->A->nrows && At->nnz == s->A->nnz);
    if (s->At == At) return MK_OK;                           // (re-setting the same operator must not release it)
    At->dependents += 1;                                     // take the new reference first, then drop the old one
    if (s->At) mk_release_operand(s->At);
    s->At = At;
    return MK_OK;
}

extern "C" int mk_csr_set_row_block(mk_csr *A, int on) {
    MK_ARG(A != nullptr);
    if (on && A->ex.mode >= 0)
        return mk_fail(MK_ERR_STATE, "mk_csr_set_row_block: the matrix already carries a halo / all-gather exchange plan");
    if (on < 0 || on > 2) return mk_fail(MK_ERR_ARG, "mk_csr_set_row_block: mode must be 0, 1 or 2");
    A->row_block = on;
    return MK_OK;
}

static bool mk_is_lls(const mk_solver *s) { return s->prm.kind >= MK_LSQR && s->prm.kind <= MK_CRAIGMR; }

__global__ __launch_bounds__(MK_BLOCK) void mk_fill_kernel(double *v, int64_t n, double a) {
    for (int64_t i = (int64_t)blockIdx.x * MK_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MK_BLOCK) v[i] = a;
}

// ------------------------------------------------------------------ device objects (MkDeviceOp, mk_solver.h)
int MkDeviceOp::init_nohalt(hipStream_t stream) {
    if (hipMalloc((void **)&d_nohalt, 2 * sizeof(int)) != hipSuccess || hipMemsetAsync(d_nohalt, 0, 2 * sizeof(int), stream) != hipSuccess) {
        (void)hipGetLastError();
        return mk_fail(MK_ERR_HIP, "out of device memory for the halt words of a device object");
    }
    return MK_OK;
}

// (an L-BFGS operator has n >= 1, so that `n == 0 ||` asks of it what mk_lbfgs_apply always asked: both pointers)
int MkDeviceOp::apply_standalone(const MkDeviceOp *F, const double *in_dev, double *out_dev) {
    MK_REQUIRE_INIT();
    MK_ARG(F && (F->n == 0 || (in_dev && out_dev)));
    MK_ARG(MK_ALIGNED16(in_dev) && MK_ALIGNED16(out_dev));
    return F->enqueue(in_dev, out_dev, mk_ctx().stream, nullptr, nullptr);
}

int mk_solver::attach(MkPrecon &into, const MkPrecon &next, const char *who, const char *name) {
    const char *noun = next.kind == MK_PRECON_OBJECT ? next.obj->noun() : "";
    // what the kind asks of the solver's operator (only a diagonal or a device matrix may be rank local) and of its own size
    if (next.kind == MK_PRECON_HOST && A->ex.mode >= 0)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: host preconditioner callbacks are single-GPU (the vector would have to be "
                       "gathered)", who);
    if (next.kind == MK_PRECON_OBJECT && A->ex.mode >= 0)
        return mk_fail(MK_ERR_UNSUPPORTED, "%s: a device %s is single-GPU (the solver's operator carries an exchange plan)",
                       who, noun);
    if (next.kind == MK_PRECON_OBJECT && next.obj->n != into.len)
        return mk_fail(MK_ERR_ARG, "%s: the %s has %lld rows, %s takes vectors of %lld entries", who, noun,
                       (long long)next.obj->n, name, (long long)into.len);
    if (next.kind == MK_PRECON_CSR && (next.op->nrows != into.len || next.op->ncols != into.len || next.op->ex.mode >= 0))
        return mk_fail(MK_ERR_ARG, "%s: %s must be a square device operator of the (local) size %lld without an exchange "
                       "plan, got %lld x %lld", who, name, (long long)into.len, (long long)next.op->nrows,
                       (long long)next.op->ncols);
    const size_t len = (size_t)(into.len > 0 ? into.len : 1);
    if (next.general() && !into.ones) {                      // (kept until the solver dies)
        MK_HIP(hipMalloc((void **)&into.ones, sizeof(double) * len + 16));
        hipLaunchKernelGGL(mk_fill_kernel, dim3(512), dim3(MK_BLOCK), 0, stream, into.ones, (int64_t)len, 1.0);
        MK_HIP(hipGetLastError());
    }
    if (next.kind == MK_PRECON_HOST && !h_pin) {             // (one pair of pinned buffers serves both slots)
        const int64_t longest = slot[0].len > slot[1].len ? slot[0].len : slot[1].len;
        const size_t cap = (size_t)(longest > 0 ? longest : 1);
        MK_HIP(hipHostMalloc((void **)&h_pin, sizeof(double) * cap, hipHostMallocDefault));
        MK_HIP(hipHostMalloc((void **)&h_pout, sizeof(double) * cap, hipHostMallocDefault));
    }
    // only the square solvers precondition a vector in place; M and N are applied out of place (mk_lls.hip)
    if (next.kind == MK_PRECON_CSR && !mk_is_lls(this) && !d_ptmp) MK_HIP(hipMalloc((void **)&d_ptmp, sizeof(double) * len + 16));
    // take the new reference first, then drop the old one: re-setting the attached object must not free it
    next.hold();
    into.release();
    into.kind = next.kind;
    into.fn = next.fn;
    into.user = next.user;
    into.op = next.op;
    into.obj = next.obj;
    into.d = next.general() ? into.ones : next.d;
    return MK_OK;
}

int mk_set_precon(mk_solver *s, int side, const MkPrecon &next, const char *who) {
    MK_ARG(s);
    if (side < 0) {
        if (!s->takes_precon())                              // (its slot is empty and stays so: nothing to remove)
            return next.kind == MK_PRECON_NONE ? (int)MK_OK
                                               : mk_fail(MK_ERR_UNSUPPORTED, "%s: this solver kind has no preconditioner hook", who);
        return s->attach(s->slot[0], next, who, "the preconditioner");
    }
    MK_ARG(side == MK_LLS_SIDE_M || side == MK_LLS_SIDE_N);
    if (!mk_is_lls(s)) return mk_fail(MK_ERR_UNSUPPORTED, "%s: not a least-squares solver", who);
    return s->attach(s->slot[side], next, who, side == MK_LLS_SIDE_N ? "N" : "M");
}

// Every setter REPLACES whatever its slot held; a NULL argument leaves the slot empty.  (The two setters of a kind of device
// object live with its type.)
extern "C" int mk_solver_set_precon_diag(mk_solver *s, const double *diag) {
    MK_ARG(MK_ALIGNED16(diag));
    return mk_set_precon(s, -1, MkPrecon::diagonal(diag), "mk_solver_set_precon_diag");
}

extern "C" int mk_solver_set_precon_callback(mk_solver *s, mk_precon_fn fn, void *user) {
    return mk_set_precon(s, -1, MkPrecon::callback(fn, user), "mk_solver_set_precon_callback");
}

extern "C" int mk_solver_set_precon_csr(mk_solver *s, const mk_csr *M) {
    return mk_set_precon(s, -1, MkPrecon::matrix(M), "mk_solver_set_precon_csr");
}

// The two-sided setters: a side that is given something takes it in place of what it held; a side that is given NULL
// loses what THIS setter attaches (a diagonal here, a callback below) and keeps anything else.
extern "C" int mk_solver_set_lls_precon(mk_solver *s, const double *diag_m, const double *diag_n) {
    MK_ARG(s);
    MK_ARG(MK_ALIGNED16(diag_m) && MK_ALIGNED16(diag_n));
    if (!mk_is_lls(s)) return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_set_lls_precon: not a least-squares solver");
    const double *diag[2] = {diag_m, diag_n};
    for (int side = 0; side < 2; ++side) {
        if (!diag[side] && s->slot[side].kind != MK_PRECON_DIAG) continue;
        const int rc = mk_set_precon(s, side, MkPrecon::diagonal(diag[side]), "mk_solver_set_lls_precon");
        if (rc != MK_OK) return rc;
    }
    return MK_OK;
}

extern "C" int mk_solver_set_lls_precon_callback(mk_solver *s, mk_precon_fn fn_m, void *user_m, mk_precon_fn fn_n,
                                                 void *user_n) {
    MK_ARG(s);
    if (!mk_is_lls(s)) return mk_fail(MK_ERR_UNSUPPORTED, "mk_solver_set_lls_precon_callback: not a least-squares solver");
    const mk_precon_fn fn[2] = {fn_m, fn_n};
    void *const user[2] = {user_m, user_n};
    for (int side = 0; side < 2; ++side) {
        if (!fn[side] && s->slot[side].kind != MK_PRECON_HOST) continue;
        const int rc = mk_set_precon(s, side, MkPrecon::callback(fn[side], user[side]), "mk_solver_set_lls_precon_callback");
        if (rc != MK_OK) return rc;
    }
    return MK_OK;
}

extern "C" int mk_solver_set_lls_precon_csr(mk_solver *s, int side, const mk_csr *P) {
    return mk_set_precon(s, side, MkPrecon::matrix(P), "mk_solver_set_lls_precon_csr");
}

extern "C" int mk_solver_destroy(mk_solver *s) {
    delete s;
    return MK_OK;
}

extern "C" int mk_solver_setup(mk_solver *s, const double *rhs, const double *guess) {
    MK_ARG(s && (rhs || s->prm.kind == MK_TRLAN || s->prm.kind == MK_LOBPCG || s->prm.kind == MK_TRSVD));   // (the eigensolvers: no start selects the hashed one)
    MK_ARG(MK_ALIGNED16(rhs) && MK_ALIGNED16(guess));        // borrowed vectors are read in 16-byte pairs
    s->q = 0;
    s->it = 0;
    s->halted = false;
    s->hist.clear();
    s->hist2.clear();
    s->hist_drained = 0;
    s->spmv_ms = 0.0;
    s->spmv_timed = 0;
    MK_HIP(hipMemsetAsync(s->d_halt, 0, 2 * sizeof(int), s->stream));
    MK_HIP(hipMemsetAsync(s->d_status, 0, sizeof(MkStatus), s->stream));
    MK_HIP(hipMemsetAsync(s->d_scal, 0, sizeof(double) * MK_NSCAL, s->stream));
    MK_HIP(hipMemsetAsync(s->d_part, 0, sizeof(double) * MK_NDOT * MK_MAXP, s->stream));
    mk_ctx().pending_rc = MK_OK;                             // (a failure of an earlier solve was reported there)
    int rc = s->setup(rhs, guess);
    if (rc != MK_OK) {
        mk_ctx().pending_rc = MK_OK;
        return rc;
    }
    MK_HIP(hipGetLastError());
    if (mk_ctx().pending_rc != MK_OK) {
        rc = mk_ctx().pending_rc;
        mk_ctx().pending_rc = MK_OK;
        return rc;
    }
    s->is_setup = true;
    return s->poll();
}

extern "C" int mk_solver_iterate(mk_solver *s, int64_t max_iters, int64_t *iters_done) {
    MK_ARG(s && max_iters >= 0);
    return s->iterate(max_iters, iters_done);
}

extern "C" int mk_solver_finish(mk_solver *s, mk_result *res) {
    MK_ARG(s && res);
    if (!s->is_setup) return mk_fail(MK_ERR_STATE, "mk_solver_finish before mk_solver_setup");
    return s->finish(res);
}

extern "C" int mk_solver_x(const mk_solver *s, const double **x_dev) {
    MK_ARG(s && x_dev);
    *x_dev = s->x();
    return MK_OK;
}

extern "C" int mk_solver_fused(const mk_solver *s, int32_t *fused) {
    MK_ARG(s && fused);
    *fused = s->is_fused() ? 1 : 0;
    return MK_OK;
}

extern "C" int mk_solver_unapplied(const mk_solver *s, int64_t *count) {
    MK_ARG(s && count);
    *count = s->unapplied();
    return MK_OK;
}

static int mk_copy_history(const std::vector<double> &hist, double *hist_host, int64_t cap) {
    MK_ARG(cap == 0 || hist_host);
    int64_t cnt = (int64_t)hist.size();
    if (cnt > cap) cnt = cap;
    memcpy(hist_host, hist.data(), sizeof(double) * (size_t)cnt);
    return MK_OK;
}

extern "C" int mk_solver_history(const mk_solver *s, double *hist_host, int64_t cap) {
    MK_ARG(s);
    return mk_copy_history(s->hist, hist_host, cap);
}

extern "C" int mk_solver_history2(const mk_solver *s, double *hist_host, int64_t cap) {
    MK_ARG(s);
    return mk_copy_history(s->hist2, hist_host, cap);
}

extern "C" int mk_solver_vector(const mk_solver *s, int index, const double **v_dev, int64_t *len) {
    MK_ARG(s && v_dev);
    const double *v = s->vector(index);
    if (!v) return mk_fail(MK_ERR_ARG, "mk_solver_vector: index %d is not defined for this solver", index);
    *v_dev = v;
    if (len) *len = s->vector_len(index);
    return MK_OK;
}

extern "C" int mk_solver_time_spmv(mk_solver *s, int64_t launches, double *avg_us) {
    return mk_solver_time_product(s, 0, launches, avg_us);
}

extern "C" int mk_solver_time_product(mk_solver *s, int which, int64_t launches, double *avg_us) {
    MK_ARG(s && launches > 0 && avg_us && which >= 0);
    if (!s->is_setup) return mk_fail(MK_ERR_STATE, "mk_solver_time_product before mk_solver_setup");
    int rc = s->enqueue_spmv_only(which);                  // one untimed launch first
    if (rc != MK_OK) return rc;
    MK_HIP(hipEventRecord(s->ev0, s->stream));
    for (int64_t k = 0; k < launches; ++k)
        if ((rc = s->enqueue_spmv_only(which)) != MK_OK) return rc;
    MK_HIP(hipEventRecord(s->ev1, s->stream));
    MK_HIP(hipEventSynchronize(s->ev1));
    MK_HIP(hipGetLastError());
    float ms = 0.f;
    MK_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    *avg_us = 1e3 * (double)ms / (double)launches;
    return MK_OK;
}

extern "C" int mk_solver_timing(const mk_solver *s, double *iterate_ms, double *spmv_ms, int64_t *spmv_launches) {
    MK_ARG(s != nullptr);
    if (iterate_ms) *iterate_ms = s->last_iterate_ms;
    if (spmv_ms) *spmv_ms = s->spmv_ms;
    if (spmv_launches) *spmv_launches = s->spmv_timed;
    return MK_OK;
}

extern "C" int mk_solver_solve(mk_solver *s, const double *rhs, const double *guess, mk_result *res) {
    int rc = mk_solver_setup(s, rhs, guess);
    if (rc != MK_OK) return rc;
    while (!s->halted) {
        rc = s->iterate((int64_t)1 << 20, nullptr);
        if (rc != MK_OK) return rc;
    }
    return mk_solver_finish(s, res);
}
