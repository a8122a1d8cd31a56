// pcg.cpp — vamp::precondCG_solver (src/vamp.cpp:664-757) for several
// independent systems (tau*A^T A + gam2*I) mu = v that share the operator.
//
// Per CG step and per still-active system, exactly the reference's scalar
// recurrences: alpha = <r,z>/<d,p>; mu += alpha p; [Onsager stop on
// gam2<v,mu>]; r -= d alpha; z = r/diag; beta = pow(<r,z>_old,-1)*<r,z>_new;
// p = z + beta p; stop when ||r||/||v|| < tol.  What is shared is the pass
// over X, so two systems cost max(k1, k2) steps instead of k1 + k2, with
// every iterate bitwise equal to a solo solve.
//
// pcg_run is pcg_check (every argument rule, before anything is queued), then
// pcg_start (the initial residual, the device-side CgState), then one of
// * TwoPassSolve (K <= 4): lmmse_mult(p) for all systems is one A.x and one
//   A^T.u launch with K right-hand sides per step;
// * OnePassSolve (K <= 2, the operator planned): A r0 by one A.x pass, then
//   one pass over X per step (vk::atax); the head start, the pre-step (the
//   slot rule, or two a solve in a third operator slot: DESIGN.md 4.9) and,
//   on several ranks, the folded decisions live here.
//
// The step's scalar decisions run on the device (vk::cg_decide), so the host
// never stands between two steps (cg_loop): it queues step i+1 (every launch
// gated on "some system still active") and only then waits for step i's flag.
// The direction update p = z + beta p rides in the next step's kernels.  A
// step queued after the last system stopped does nothing; its launches are
// dropped from the stats.
#include <algorithm>
#include <cstddef>
#include <string>

#include "ctx.h"

// device addresses of CgState fields
template <class T>
static T* field(vk::CgState* cs, size_t off) {
    return reinterpret_cast<T*>(reinterpret_cast<char*>(cs) + off);
}

// The outcome of a decided CG step as the host reads it.
struct CgOutcome {
    int any = 0;
    bool pre = false;  // some decided step's launches made the pre-step (packed words only)
    int iters[vk::kMaxRhs] = {};
};

// Flag words (of the context's mapped block) of the packed decisions: step i
// is published into word kCgPackWord + (i & 1), so step i+1's (queued before
// the host reads step i's) never overwrites the one the host is waiting for.
static constexpr int kCgPackWord = 2;

// Both readers wait for the decision of step `step` (sequence seq) and read it
// into *o, which holds the outcome of the step before; the next step, queued
// before the wait, writes the other word / slot.
// packed (the one-pass form, K <= 2): the decision is ONE word (vk::cg_pack)
// in flag word kCgPackWord + (step & 1)
static vampomi_status read_packed(vampomi_ctx* c, int step, unsigned long long seq, CgOutcome* o) {
    const int word = kCgPackWord + (step & 1);
    STCHK(wait_flag(c, seq << 32, word));  // the step decided and published
    STCHK(op_check_err(c));                // (its decision is void if its operator launch timed out)
    const unsigned long long w = __atomic_load_n(c->h_flag + word, __ATOMIC_ACQUIRE);
    if ((w >> 32) != (seq & 0xffffffffULL))
        return fail(VAMPOMI_ERR_STATE, "CG step " + std::to_string(step) + ": decision word holds sequence " +
                                           std::to_string(w >> 32) + ", expected " + std::to_string(seq));
    o->any = (int)((w >> 30) & 1);
    o->pre = o->pre || (w & vk::kCgPackPre) != 0;
    o->iters[0] = (int)(w & 0x7fff);
    o->iters[1] = (int)((w >> 15) & 0x7fff);
    return VAMPOMI_OK;
}
// else (K up to 4): the decision's own mirror slot (step & 1), tagged with its flag value
static vampomi_status read_mirror(vampomi_ctx* c, int step, unsigned long long seq, CgOutcome* o) {
    STCHK(wait_flag(c, seq));  // the step decided
    STCHK(op_check_err(c));    // (its decision is void if its operator launch timed out)
    const vk::CgMirror* m = c->h_cgm + (step & 1);
    if (__atomic_load_n(&m->seq, __ATOMIC_ACQUIRE) != seq)
        return fail(VAMPOMI_ERR_STATE, "CG step " + std::to_string(step) + ": decision slot holds sequence " +
                                           std::to_string(m->seq) + ", expected " + std::to_string(seq));
    o->any = m->any;
    for (int k = 0; k < vk::kMaxRhs; ++k) o->iters[k] = m->iters[k];
    return VAMPOMI_OK;
}

// the host loop shared by both forms: queue step i+1 (solve.enqueue), then
// wait for step i's decision; a step queued after the last system stopped is
// dropped from the stats.  *last: the last decided step's outcome (its
// iteration counts are final).  solve.settle() is called instead of enqueue(i)
// when no step i is queued (i = max_iter), for a decision of step i-1 that
// step i's launch would have formed (folded decisions)
// *nrun (may be null): the steps that ran (every awaited step did)
template <class Solve>
static vampomi_status cg_loop(vampomi_ctx* c, int max_iter, bool packed, Solve& solve, CgOutcome* last,
                              int* nrun = nullptr) {
    unsigned long long prev = 0, cur = 0;
    STCHK(solve.enqueue(0, &prev));
    for (int i = 1;; ++i) {
        const size_t mark = c->pending.size();
        const vampomi_stats before = c->stats;
        if (i < max_iter)
            STCHK(solve.enqueue(i, &cur));
        else
            STCHK(solve.settle());
        c->stats.host_syncs++;
        STCHK(packed ? read_packed(c, i - 1, prev, last) : read_mirror(c, i - 1, prev, last));
        if (!last->any || i >= max_iter) {
            if (i < max_iter) drop_launches(c, mark, before);  // step i was queued in vain: it did nothing
            if (nrun) *nrun = i;
            break;
        }
        prev = cur;
    }
    return VAMPOMI_OK;
}

// What the phases of one solve share.
struct Pcg {
    vampomi_ctx* c;
    const std::vector<CgSystem*>& sys;
    const PcgArgs& a;
    int K;
    double diag;  // :676-677
    bool rec;     // some system keeps W = A^T A mu (then every system has its raw-product slot S)
    // set by pcg_start, once the operator is planned:
    bool op1 = false;   // the one-pass form
    bool head = false;  // the head start (ctx.h, HeadStart) runs
    bool pre_ok = false;  // the pre-step can be made or used: one rank, team plans, packed decisions
    bool pre2 = false;  // system 0's step 1 composed, its step 2 in the head pass
    int J = 0;          // system 0's composed steps (pre2: 1, or 2 in mode 3); step J + 1 in the head pass
    const double* xnext() const { return a.hs ? a.hs->xnext : nullptr; }
    const int* gate() const { return field<int>(c->cgs, offsetof(vk::CgState, any)); }
    const double* beta() const { return field<double>(c->cgs, offsetof(vk::CgState, beta)); }
    // a reduction into scal[slot...], gated on *g
    vk::RedOut red(int slot, const int* g) const {
        return vk::RedOut{c->red_part, c->scal + slot, c->ticket, nullptr, 0, g};
    }
};

static vampomi_status copy_nvec(vampomi_ctx* c, double* dst, const double* src) {
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)c->N * 8, hipMemcpyDeviceToDevice, c->st));
    return VAMPOMI_OK;
}

// out = A x for n products by ONE A.x pass into buf's ld-rows (nothing if
// n = 0); a product whose out is not its row of buf is copied there
struct Product {
    const double* x;
    double* out;
};
static vampomi_status ax_products(vampomi_ctx* c, int n, const Product* pr, double* buf) {
    if (n == 0) return VAMPOMI_OK;
    const double* px[vk::kMaxRhs];
    for (int j = 0; j < n; ++j) px[j] = pr[j].x;
    STCHK(ax_dev(c, n, px, buf));
    for (int j = 0; j < n; ++j)
        if (pr[j].out != buf + (int64_t)j * c->ld) STCHK(copy_nvec(c, pr[j].out, buf + (int64_t)j * c->ld));
    return VAMPOMI_OK;
}
// A extra_x and A xnext when no CG step carries them
static vampomi_status extra_alone(const Pcg& s) {
    Product pr[2];
    int n = 0;
    if (s.a.extra_x) pr[n++] = {s.a.extra_x, s.a.ex_out};
    if (s.xnext()) pr[n++] = {s.xnext(), s.a.hs->axnext};
    return ax_products(s.c, n, pr, s.a.nscratch);
}

// the vectors every CG kernel takes; step: those of cg_update too
static vk::CgVecs fill_vecs(const Pcg& s, bool step) {
    vk::CgVecs cv{};
    cv.tau = s.a.tau;
    cv.gam2 = s.a.gam2;
    for (int k = 0; k < s.K; ++k) {
        const CgSystem* y = s.sys[k];
        cv.mu[k] = y->mu;
        cv.r[k] = y->r;
        cv.z[k] = y->z;
        cv.p[k] = y->p;
        cv.v[k] = y->v;
        if (!step) continue;
        cv.d[k] = y->d;
        cv.W[k] = y->W;
        cv.S[k] = y->W ? y->S : nullptr;
        cv.AW[k] = y->AW;
    }
    return cv;
}

// the solve's outputs from the last decided step
static void store_iters(const Pcg& s, const CgOutcome& last) {
    for (int k = 0; k < s.K; ++k) {
        s.sys[k]->iters = last.iters[k];
        if (s.a.ref_passes) *s.a.ref_passes += 2 * (int64_t)s.sys[k]->iters;
    }
}

// Every rule on pcg_run's arguments, before anything is queued.
static vampomi_status pcg_check(const vampomi_ctx*, const std::vector<CgSystem*>& sys, const PcgArgs& a) {
    const int K = (int)sys.size();
    if (K < 1 || K > vk::kMaxRhs) return fail(VAMPOMI_ERR_ARG, "pcg: 1..4 systems");
    if (a.extra_x && (!a.ex_out || K + 1 >= vk::kMaxRhs)) return fail(VAMPOMI_ERR_ARG, "pcg: extra A.x needs K <= 2");
    if (a.hs && (!a.onepass || K != 2 || !a.extra_x || a.ar0 || sys[0]->mu0_nonzero ||
                 (a.hs->xnext && !a.hs->axnext)))
        return fail(VAMPOMI_ERR_ARG, "pcg: the head start needs the one-pass form, two systems, extra_x, "
                                     "system 0 from zero and no ar0");
    bool lmmse = false, rec = false;  // some start needs its lmmse pass; some system keeps W
    for (const CgSystem* y : sys) {
        lmmse = lmmse || (y->mu0_nonzero && !y->atx0);
        rec = rec || y->W;
    }
    if (lmmse && a.pm != PreMode::normal) return fail(VAMPOMI_ERR_ARG, "pcg: a start queued ahead needs no lmmse pass");
    if (a.pre && a.init) return fail(VAMPOMI_ERR_ARG, "pcg: the prelude rides only in the device-side start");
    if (a.pm != PreMode::normal && !a.pre) return fail(VAMPOMI_ERR_ARG, "pcg: a start queued ahead is the prelude's");
    if (a.pm != PreMode::normal && (a.pm == PreMode::ahead) != (a.pre->dev.scal != nullptr))
        return fail(VAMPOMI_ERR_ARG, "pcg: a start queued ahead needs the prelude and its device scalars");
    if (a.max_iter <= 0) return VAMPOMI_OK;  // (no step runs: the rest is about the steps)
    for (int k = 0; a.onepass && K <= vk::kOpMaxK && a.ar0 && k < K; ++k)  // (the two-pass form ignores ar0)
        if (a.ar0[k] && sys[k]->mu0_nonzero) return fail(VAMPOMI_ERR_ARG, "pcg: A r0 given for a nonzero start");
    for (const CgSystem* y : sys)  // (the kernels store all K raw products or none)
        if (rec && !y->S) return fail(VAMPOMI_ERR_ARG, "pcg: W needs an S scratch vector for every system");
    return VAMPOMI_OK;
}

// The start: r = v - lmmse_mult(mu0) (:681-684), z, p, <r,z>, <v,v> and the
// device-side CgState; plans the operator and with it the form of the solve
// (s.op1, head, pre_ok, pre2).  *go: the solve goes on (not when the start is
// only queued ahead, nor when no step runs)
static vampomi_status pcg_start(Pcg& s, bool* go) {
    vampomi_ctx* c = s.c;
    const PcgArgs& a = s.a;
    const HeadStart* hs = a.hs;
    const int K = s.K;
    *go = false;
    {
        const double* vv[vk::kMaxRhs];
        double* dd[vk::kMaxRhs];
        int n = 0;
        for (CgSystem* y : s.sys) {
            if (y->mu0_nonzero && !y->atx0) vv[n] = y->mu, dd[n++] = y->d;
            if (y->mu0_nonzero && a.ref_passes) *a.ref_passes += 2;
        }
        if (n > 0) STCHK(lmmse_dev(c, n, vv, dd, a.tau, a.gam2, a.nscratch));
    }
    if (a.onepass && K <= vk::kOpMaxK && c->have_X) STCHK(op_prepare(c));
    s.op1 = a.onepass && K <= vk::kOpMaxK && c->have_X && c->op_ok;
    // the head start: system 0's first step rides in the pass that starts the
    // solve; it is then one step ahead (CgState.off).  hs_ok: agreed, hs_on included
    s.head = hs && hs->abern && c->hs_ok && c->op_ok && a.max_iter > 0;
    s.pre_ok = hs && s.op1 && !c->use_comm && c->opp.T >= 1 && hs->T1 && hs->U1 && hs->pre_done && a.max_iter > 0 &&
               a.max_iter < vk::kCgPackMaxIter;
    s.pre2 = s.head && s.pre_ok && hs->pre_have;
    s.J = !s.pre2 ? 0 : hs->pre3 && hs->n_have >= 2 ? 2 : 1;
    vk::CgVecs cv = fill_vecs(s, false);
    for (int k = 0; k < K; ++k) {
        const CgSystem* y = s.sys[k];
        cv.atx0[k] = y->mu0_nonzero ? y->atx0 : nullptr;
        cv.d[k] = (y->mu0_nonzero && !y->atx0) ? y->d : nullptr;
    }
    vk::CgState s0{};
    s0.K = K;
    s0.gam2 = a.gam2;
    s0.tol = a.tol;
    s0.maxit = a.max_iter;
    s0.off[0] = s.head ? 1 + s.J : 0;
    s0.any = a.max_iter > 0 ? 1 : 0;
    for (int k = 0; k < K; ++k) {
        s0.active[k] = 1;
        s0.onsager[k] = s.sys[k]->onsager ? 1 : 0;
        s.sys[k]->iters = 0;
    }
    if (a.init) {  // the caller's reductions resolve together with <r,z>, <v,v> (one host wait)
        std::vector<double> rzvv(2 * K);
        vk::RedOut ro{};
        STCHK(a.init->sink(2 * K, true, rzvv.data(), &ro));
        HIPCHK(vk::cg_init(K, c->M, cv, s.diag, ro, c->st));
        STCHK(a.init->flush());
        for (int k = 0; k < K; ++k) {
            s0.rz[k] = rzvv[2 * k];
            s0.vv[k] = rzvv[2 * k + 1];
        }
        if (a.max_iter <= 0) return extra_alone(s);
        HIPCHK(vk::cg_start(s0, c->cgs, c->st));
    } else if (a.pm != PreMode::queued) {
        // <r,z>, <v,v> stay on the device: the CgState is built there, no host wait.
        // pre: the caller's prelude rides in the same launch, and on one rank
        // that launch's last block also builds the CgState (three launches in one).
        // (queued: all this was queued ahead by the previous iteration, scalars
        // from the device: the prelude, and on several ranks the sums'
        // all-reduce and the CgState)
        const vk::RedOut ro = s.red(SL_CGI, nullptr);
        const bool own_start = a.pre && !c->use_comm;
        if (a.pre)
            HIPCHK(vk::prelude_cg_init(K, c->M, *a.pre, cv, s.diag, ro, own_start ? &s0 : nullptr, c->cgs, c->st));
        else
            HIPCHK(vk::cg_init(K, c->M, cv, s.diag, ro, c->st));
        if (!own_start) {
            STCHK(allreduce_dev(c, c->scal + SL_CGI, (size_t)(2 * K)));
            // (ahead: gam2 from the device, the prelude's scalars {eta1, gam2, ...})
            if (a.max_iter > 0)
                HIPCHK(vk::cg_start_from(s0, c->scal + SL_CGI, c->cgs, c->st,
                                         a.pm == PreMode::ahead ? a.pre->dev.scal + 1 : nullptr));
        }
        if (a.pm == PreMode::ahead) return VAMPOMI_OK;
    }
    if (a.max_iter <= 0) return extra_alone(s);
    *go = true;
    return VAMPOMI_OK;
}

// ---- one pass over X per CG step (vk::atax) ----
// A r0 for every system (and A extra_x) by one A.x pass; then each step
// forms q = A p = A r/diag + beta*q_old on the fly, streams X once for
// d = tau*A^T q + gam2*p and A d, and cg_update carries A r -= alpha*A d
struct OnePassSolve : Pcg {
    HeadStart* const hs;
    // A r, q = A p and A d of the systems: N-vectors of op_nvec
    double* const AR;
    double* const Q;
    const double* const AD;
    vk::CgVecs cu;  // cg_update's vectors (from the first regular step on with the pre-step's, where offered)
    // several ranks, team plans: each step's decision is formed by the next
    // operator launch (vk::OpFold) from the all-reduced sums, instead of by
    // a decision launch of its own; the two CgStates alternate (the launch
    // reads one while its workgroup 0 writes the other).  cur: the state
    // the next launches use; pend: the decision not yet formed
    const bool fold;
    int cur = 0;
    vk::OpFold pend;
    // the decisions travel as one packed word each (read_packed): one
    // system-scope store instead of the mirror's six, a drain and the flag
    const bool packed;
    bool offer = false;  // the pre-step for the next solve: offered to every regular step
    unsigned long long token = 0;
    bool offer3 = false;  // mode 3: the next solve's two pre-steps in the third slot of steps 0 and 1
    int nrun = 0;         // the regular steps that ran

    explicit OnePassSolve(const Pcg& s)
        : Pcg(s), hs(a.hs), AR(c->op_nvec), Q(AR + (int64_t)vk::kMaxRhs * c->ld),
          AD(AR + (int64_t)2 * vk::kMaxRhs * c->ld), cu(fill_vecs(s, true)),
          fold(c->use_comm && c->cg_fold && c->opp.T >= 1 && (!head || c->opp_hs.T >= 1)),
          packed(K <= 2 && a.max_iter < vk::kCgPackMaxIter) {
        cu.nA = c->N;
        for (int k = 0; k < K; ++k) {
            cu.Q[k] = Q + (int64_t)k * c->ld;
            // (head start: A r0 of system 0 is hs->abern (r0 = v), used in place as its A r)
            cu.AR[k] = head && k == 0 ? hs->abern : AR + (int64_t)k * c->ld;
            cu.AD[k] = AD + (int64_t)k * c->ld;
        }
        if (!c->use_comm) {  // one rank: cg_update sums the operator's A d slots itself
            cu.adpart = c->op_part;
            cu.adld = c->ld;
            cu.adslots = c->opp.nslots;
        }
        // the division of A d by sqrt(N) happens where cg_update reads it
        // (several ranks: the all-reduced A d, op_dev(..., divide = false))
        cu.addiv = c->sqrtN;
    }
    vk::CgState* state(int i) const { return c->cgs + i; }
    // the operator's arguments, and those of system k
    vk::OpArgs op_args() const {
        vk::OpArgs o{};
        o.beta = beta();
        o.diag = diag;
        o.tau = a.tau;
        o.gam2 = a.gam2;
        return o;
    }
    void op_system(vk::OpArgs& o, int k) const {
        o.ar.p[k] = cu.AR[k];
        o.qo.p[k] = cu.Q[k];
        o.p.p[k] = sys[k]->p;
        o.z.p[k] = sys[k]->z;
        o.d.p[k] = sys[k]->d;
        o.sraw.p[k] = rec ? sys[k]->S : nullptr;
    }

    // A r0 of the systems that do not bring it (a.ar0; zero starts, r0 = v),
    // A extra_x and A xnext by one A.x pass: straight into AR when no system
    // brings its own, else by way of nscratch.  (With the head start its launch
    // forms them: head_step)
    vampomi_status first_products() {
        Product pr[vk::kMaxRhs];
        int n = 0;
        bool given = false;
        for (int k = 0; k < K; ++k) {
            if (a.ar0 && a.ar0[k]) {
                given = true;
                STCHK(copy_nvec(c, AR + (int64_t)k * c->ld, a.ar0[k]));
            } else {
                pr[n++] = {sys[k]->r, AR + (int64_t)k * c->ld};
            }
        }
        if (a.extra_x) pr[n++] = {a.extra_x, a.ex_out};
        if (xnext()) pr[n++] = {xnext(), hs->axnext};
        return ax_products(c, n, pr, given ? a.nscratch : AR);
    }

    // system 0's step 1 (it = -1 - J) from T1, U1 and A r0 = abern: no pass
    vampomi_status compose_step() {
        vk::PreCompose pc{};
        pc.T1 = hs->T1;
        pc.U1 = hs->U1;
        pc.ab = cu.AR[0];
        pc.p = sys[0]->p;
        pc.d = sys[0]->d;
        pc.S = rec ? sys[0]->S : nullptr;
        pc.AD = const_cast<double*>(cu.AD[0]);
        pc.diag = diag;
        pc.tau = a.tau;
        pc.gam2 = a.gam2;
        if (J == 2) {  // (compose_step2 forms this step's alpha from <r0,z0>)
            pc.cs = c->cgs;
            pc.rz_save = hs->rz_save;
        }
        HIPCHK(vk::pre_compose(c->M, c->N, pc, red(SL_DP, gate()), c->st));
        vk::CgVecs cp = cu;  // A d is the composed vector, whole
        cp.adpart = nullptr;
        cp.addiv = 0.0;
        vk::CgDecide dc{};  // no mirror, no flag: the host does not wait for this step
        dc.on = 1;
        dc.it = -1 - J;
        dc.mask = 1;
        HIPCHK(vk::cg_update(1, c->M, cp, diag, c->cgs, c->scal + SL_DP, nullptr, 0, red(SL_CG, gate()), dc,
                             c->st));
        hs->pre_used = true;
        hs->n_used = J;
        return VAMPOMI_OK;
    }

    // mode 3, two pre-steps in hand: system 0's step 2 (it = -2) from T1, T2,
    // U1, U2 and the scalars composed step 1 left on the device: no pass.  Its
    // direction update p1 = z1 + beta0 p0 rides in its cg_update
    vampomi_status compose_step2() {
        vk::PreCompose2 pc{};
        pc.T1 = hs->T1;
        pc.T2 = hs->T2;
        pc.U1 = hs->U1;
        pc.U2 = hs->U2;
        pc.ar = cu.AR[0];
        pc.q = cu.Q[0];
        pc.p = sys[0]->p;
        pc.z = sys[0]->z;
        pc.d = sys[0]->d;
        pc.S = rec ? sys[0]->S : nullptr;
        pc.AD = const_cast<double*>(cu.AD[0]);
        pc.diag = diag;
        pc.tau = a.tau;
        pc.gam2 = a.gam2;
        pc.cs = c->cgs;
        pc.rz_save = hs->rz_save;
        pc.dp0 = c->scal + SL_DP;
        HIPCHK(vk::pre_compose2(c->M, c->N, pc, red(SL_DP, gate()), c->st));
        vk::CgVecs cp = cu;
        cp.adpart = nullptr;
        cp.addiv = 0.0;
        vk::CgDecide dc{};
        dc.on = 1;
        dc.it = -2;
        dc.mask = 1;
        HIPCHK(vk::cg_update(1, c->M, cp, diag, c->cgs, c->scal + SL_DP, nullptr, 1, red(SL_CG, gate()), dc,
                             c->st));
        return VAMPOMI_OK;
    }

    // system 0's step 1 (it = -1: its count becomes 1 + off - 1 + ... = 1; its
    // step 2 after compose_step, whose direction update then rides in)
    // together with A r0 of system 1, A extra_x and A xnext: one pass
    vampomi_status head_step() {
        vk::OpArgs o = op_args();
        op_system(o, 0);
        o.fuse = pre2 ? 1 : 0;
        const double* xn = xnext();
        const double* px[vk::kOpPlain] = {sys[1]->r, a.extra_x, xn ? xn : a.extra_x};
        double* out[vk::kOpPlain] = {cu.AR[1], a.ex_out, xn ? hs->axnext : a.nscratch};
        STCHK(op_dev_plain(c, o, px, out, gate()));
        vk::CgVecs ch = cu;
        if (!c->use_comm) ch.adslots = (int)c->opp_hs.nslots;
        else ch.addiv = 0.0;  // (op_dev_plain divided its A d already)
        const double* dp = c->use_comm ? AD + (int64_t)(1 + vk::kOpPlain) * c->ld : c->scal + SL_DP;
        vk::CgDecide dc{};  // no mirror, no flag: the host does not wait for this step
        dc.on = !c->use_comm;
        dc.it = -1;
        dc.mask = 1;
        HIPCHK(vk::cg_update(1, c->M, ch, diag, c->cgs, dp, nullptr, pre2 ? 1 : 0, red(SL_CG, gate()), dc,
                             c->st));
        if (c->use_comm) {
            STCHK(allreduce_dev(c, c->scal + SL_CG, 3));
            if (fold) {  // formed by step 0's operator launch
                pend.on = 1;
                pend.it = -1;
                pend.mask = 1;
            } else {
                HIPCHK(vk::cg_decide(c->cgs, c->scal + SL_CG, -1, nullptr, nullptr, 0, c->st, 1));
            }
        }
        hs->used = true;
        return VAMPOMI_OK;
    }

    // queues CG step i; *seq: the sequence number its decision stores
    vampomi_status enqueue(int i, unsigned long long* seq) {
        // the direction updates fused into step i: every system's from step
        // 1 on; at step 0 those of the systems already under way (head start)
        const int fuse = i > 0 ? (1 << K) - 1 : head ? 1 : 0;
        vk::OpArgs o = op_args();
        for (int k = 0; k < K; ++k) op_system(o, k);
        // mode 3: steps 0 and 1 carry the next solve's pre-steps in a third slot
        const bool third = offer3 && i < 2;
        if (third) {
            o.alt.ar = i == 0 ? hs->axnext : hs->U1;
            o.alt.p = i == 0 ? hs->xnext : hs->T1;
            o.alt.d = i == 0 ? hs->T1 : hs->T2;
        }
        if (offer) {
            o.alt.cs = c->cgs;
            o.alt.done = hs->pre_done;
            o.alt.token = token;
            o.alt.ar = hs->axnext;
            o.alt.p = hs->xnext;
            o.alt.d = hs->T1;
        }
        o.fuse = fuse;
        const int* g = gate();
        vk::CgState* cs = c->cgs;
        if (fold) {
            o.beta = nullptr;
            if (pend.on) {  // the previous step's decision, formed by this launch into the other state
                o.fold = pend;
                o.fold.src = state(cur);
                o.fold.dst = state(cur ^ 1);
                o.fold.red = c->scal + SL_CG;
                cur ^= 1;
                pend.on = 0;
            }
            cs = state(cur);
            g = field<int>(cs, offsetof(vk::CgState, any));
            if (!o.fold.on) o.beta = field<double>(cs, offsetof(vk::CgState, beta));
        }
        STCHK(op_dev(c, third ? vk::kOpSys : K, o, g, c->use_comm, false));
        vk::CgVecs cv = cu;  // (a 3-system launch left its A d partials in its own plan's slots)
        if (third) {
            // U1 / U2: the third slot's team partials in team order, / sqrt(N)
            vk::Ptrs us{};
            us.p[0] = i == 0 ? hs->U1 : hs->U2;
            HIPCHK(vk::op_reduce(c->opp3, 1, c->N, c->ld, c->op_part, us, c->sqrtN, c->st, g, vk::kOpMaxK));
            cv.adslots = (int)c->opp3.nslots;
        }
        const double* dp = c->use_comm ? AD + (int64_t)K * c->ld : c->scal + SL_DP;
        *seq = ++c->sync_seq;
        unsigned long long* flag = packed ? c->d_flag + kCgPackWord + (i & 1) : c->d_flag;
        vk::CgMirror* mirror = packed ? nullptr : c->d_cgm;
        vk::CgDecide dc{};
        if (!c->use_comm) {
            dc.on = 1;
            dc.it = i;
            dc.mirror = mirror;
            dc.flag = flag;
            dc.seq = *seq;
            dc.pack = packed ? 1 : 0;
        }
        HIPCHK(vk::cg_update(K, c->M, cv, diag, cs, dp, nullptr, fuse, red(SL_CG, g), dc, c->st));
        if (c->use_comm) {
            STCHK(allreduce_dev(c, c->scal + SL_CG, (size_t)(3 * K)));
            if (fold) {  // formed by the next step's operator launch (or settle)
                pend.on = 1;
                pend.it = i;
                pend.mask = 0xf;
                pend.pack = packed ? 1 : 0;
                pend.mirror = mirror;
                pend.flag = flag;
                pend.seq = *seq;
            } else {
                HIPCHK(vk::cg_decide(c->cgs, c->scal + SL_CG, i, mirror, flag, *seq, c->st, 0xf, packed ? 1 : 0));
            }
        }
        return VAMPOMI_OK;
    }

    // the last step's decision when no step follows to form it
    vampomi_status settle() {
        if (!pend.on) return VAMPOMI_OK;
        HIPCHK(vk::cg_decide(state(cur), c->scal + SL_CG, pend.it, pend.mirror, pend.flag, pend.seq, c->st, pend.mask,
                             pend.pack));
        pend.on = 0;
        return VAMPOMI_OK;
    }

    vampomi_status finish(const CgOutcome& last) {
        STCHK(op_check_err(c));
        store_iters(*this, last);
        if (offer) hs->pre_made = last.pre;
        if (offer) hs->n_made = last.pre ? 1 : 0;
        if (offer3) {  // a step that ran made its pre-step
            hs->n_made = std::min(nrun, 2);
            hs->pre_made = hs->n_made > 0;
        }
        return VAMPOMI_OK;
    }

    vampomi_status run() {
        if (!head) STCHK(first_products());
        if (pre2) STCHK(compose_step());
        if (J == 2) STCHK(compose_step2());
        if (head) STCHK(head_step());
        offer = pre_ok && packed && hs->pre_offer && hs->xnext && hs->axnext && !fold;
        offer3 = offer && hs->pre3 && c->sys3_ok && hs->T2 && hs->U2;  // (K = 2: pcg_check, the head start's rule)
        if (offer3) offer = false;  // (no slot rule and no token in mode 3)
        if (offer) {
            token = ++c->pre_seq;
            cu.pre_u1 = hs->U1;
            cu.pre_done = hs->pre_done;
            cu.pre_token = token;
        }
        CgOutcome last;
        STCHK(cg_loop(c, a.max_iter, packed, *this, &last, &nrun));
        return finish(last);
    }
};

// ---- two passes over X per CG step ----
// From step 1 on, the direction update p = z + beta p (:738-739) of the step
// before is fused into the step's kernels: the A.x pass, the lmmse_mult
// epilogue and <d,p> form it on the fly, cg_update stores it.
struct TwoPassSolve : Pcg {
    vk::CgVecs cu;  // (cu.AS: this step's A p, the A.x pass output in nscratch's rows)
    double* dd[vk::kMaxRhs];
    double* ss[vk::kMaxRhs];
    // several ranks: <d,p> rides in the A.x all-reduce (nscratch holds K*ld + K);
    // c->dp_separate keeps the one-rank form (tests compare bitwise)
    const bool split_dp;

    explicit TwoPassSolve(const Pcg& s)
        : Pcg(s), cu(fill_vecs(s, true)), split_dp(c->use_comm && K < vk::kMaxRhs && !c->dp_separate) {
        for (int k = 0; k < K; ++k) {
            dd[k] = sys[k]->d;
            ss[k] = sys[k]->S;
            cu.AS[k] = a.nscratch + (int64_t)k * c->ld;
            if (sys[k]->AW) cu.nA = c->N;
        }
    }

    // queues CG step i; *seq: the sequence number its decision stores
    vampomi_status enqueue(int i, unsigned long long* seq) {
        const bool fuse = i > 0;
        vk::AxFuse fu{};
        fu.gate = gate();
        if (fuse) {
            for (int k = 0; k < K; ++k) fu.z.p[k] = cu.z[k];
            fu.beta = beta();
        }
        // d = lmmse_mult(p) (:700).  One rank: <d,p> by a reduction over d and
        // p into scal[SL_DP + k].  Several ranks: <d,p> = tau*|A p|^2 +
        // gam2*|p|^2, with the local |p|^2 all-reduced together with A p's
        // partials and |A p|^2 summed over the replicated N-vector: one
        // collective per step fewer.
        // the first step's pass also carries A.extra_x (one more right-hand side)
        const double* px[vk::kMaxRhs];
        for (int k = 0; k < K; ++k) px[k] = cu.p[k];
        const bool ex = i == 0 && a.extra_x;
        if (ex) px[K] = a.extra_x;
        const int KA = ex ? K + 1 : K;
        const double* pp_dev = nullptr;
        vk::DotArgs tail{};
        if (split_dp) {
            tail.nt = K;
            for (int k = 0; k < K; ++k)
                tail.t[k] = fuse ? vk::DotTerm{cu.p[k], cu.p[k], vk::SQPUPD, cu.z[k], beta() + k}
                                 : vk::DotTerm{cu.p[k], cu.p[k], vk::DOT};
            pp_dev = a.nscratch + (int64_t)KA * c->ld;
        }
        STCHK(ax_dev(c, KA, px, a.nscratch, &fu, split_dp ? &tail : nullptr));
        if (ex) STCHK(copy_nvec(c, a.ex_out, a.nscratch + (int64_t)K * c->ld));
        if (split_dp) {
            vk::DotArgs uu{};
            uu.nt = K;
            for (int k = 0; k < K; ++k) uu.t[k] = vk::DotTerm{cu.AS[k], cu.AS[k], vk::DOT};
            HIPCHK(vk::dots(uu, c->N, red(SL_DP, gate()), c->st));
        }
        STCHK(atx_dev(c, K, cu.AS, dd, 1, a.tau, a.gam2, cu.p, gate(), fuse ? cu.z : nullptr, beta(), !split_dp,
                      rec ? ss : nullptr));
        *seq = ++c->sync_seq;
        vk::CgDecide dc{};
        if (!c->use_comm) {  // one rank: cg_update's last block decides
            dc.on = 1;
            dc.it = i;
            dc.mirror = c->d_cgm;
            dc.flag = c->d_flag;
            dc.seq = *seq;
        }
        HIPCHK(vk::cg_update(K, c->M, cu, diag, c->cgs, c->scal + SL_DP, pp_dev, fuse ? (1 << K) - 1 : 0,
                             red(SL_CG, gate()), dc, c->st));
        if (c->use_comm) {  // the sums are final after the all-reduce
            STCHK(allreduce_dev(c, c->scal + SL_CG, (size_t)(3 * K)));
            HIPCHK(vk::cg_decide(c->cgs, c->scal + SL_CG, i, c->d_cgm, c->d_flag, *seq, c->st));
        }
        return VAMPOMI_OK;
    }
    vampomi_status settle() { return VAMPOMI_OK; }

    vampomi_status run() {
        if (xnext()) {  // (no one-pass plan: the head start's next product by its own pass)
            const Product pr{xnext(), a.hs->axnext};
            STCHK(ax_products(c, 1, &pr, a.nscratch));
        }
        CgOutcome last;
        STCHK(cg_loop(c, a.max_iter, false, *this, &last));
        store_iters(*this, last);
        return VAMPOMI_OK;
    }
};

vampomi_status pcg_run(vampomi_ctx* c, const std::vector<CgSystem*>& sys, const PcgArgs& args) {
    if (args.hs) {
        args.hs->used = args.hs->pre_made = args.hs->pre_used = false;
        args.hs->n_made = args.hs->n_used = 0;
    }
    STCHK(pcg_check(c, sys, args));
    bool rec = false;
    for (const CgSystem* y : sys) rec = rec || y->W;
    const double diag = args.tau * (double)(c->N - 1) / (double)c->N + args.gam2;  // :676-677
    Pcg s{c, sys, args, (int)sys.size(), diag, rec};
    bool go = false;
    STCHK(pcg_start(s, &go));
    if (!go) return VAMPOMI_OK;
    return s.op1 ? OnePassSolve(s).run() : TwoPassSolve(s).run();
}
