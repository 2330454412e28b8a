// loopctl_check.cpp -- the loop controller's decision (loop_verdict.hpp) in its five forms against a plain sequential statement of the
// reference's loop, bit for bit, on the CPU under the address / UB sanitizers (make loopctl_check; links nothing of HIP).
//
// A script fixes what every trial of a time step would measure: per iteration the two sums alpha_0 is formed from, how many trials
// the line search rejects, and for trial j of iteration k (the step alpha_0 / 2^j) its energy columns and its row of statistics.  The
// sequential model below walks the script as the reference does (first trial at alpha_0, halve while the energy increases, fail at
// alpha == 0, push the pair, stop at the cap or the tolerance; Optimizer.cpp:806-833, DOTTimeStepper.cpp:474-494) -- with indices and
// a `while`, sharing only lbfgs_history.hpp, which has its own check.  The slot simulator hands loop_verdict<CTL> what the kernels of a
// slot hand the controller: a new-direction slot the first trial (PAIR, where the pairing rule fires: the half step in full and the
// full step's energy; SPEC: the unit step, which is a trial of the search only when alpha_0 == 1), a retry slot the trial at DevLoop::
// alpha.  Trials the sequential search never sees are NaN throughout: a controller that used one could not agree.
// Asserted per form (PAIR and PAIR_VP with cold and with saturated pairing counters):
//   (a) after every accepted trial E_cur, g2_cur, the log, L.m and order / ys / b / sy over [0, m) -- and, while the loop goes on, xi
//       and the free slot -- and at the end iter, halvings, evals and status are the model's;
//   (b) the stop verdicts published number loop_stopped_launches(), one less in a step that collapsed;
//   (c) every slot publishes once, holdVerdict = 2 slots + stop;
//   (d) x_cur / x_trial and g_cur / g_trial swap with every accept, x once more on a collapse;
//   (e) the controller's chunk sums add up to chunked_sum().
// Every class of case the scripts are meant to hold is counted and must have occurred.
#include "loop_verdict.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

using namespace dotmi;

namespace {

// ---- scripts ----------------------------------------------------------------------------------------------------------------
struct Trial {
    double ea, ei, R[RED_K];
};
struct ScriptIter {
    double pg, pHp;
    int nrej;        // trials rejected before one is accepted; -1: none ever is (the step length runs out)
    double ea, ei;   // the accepted trial's energy columns
    double g2;       // its |g|^2
    bool ysNeg;      // its y.s <= 0
    double Eprev;    // the energy the iteration starts from
};
struct Script {
    uint64_t seed;
    int hist, iterCap, logCap;
    double tol, dtSq, alphaMin, ea0, ei0, g2_0;
    std::vector<ScriptIter> it;
};

uint64_t splitmix(uint64_t &s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double unit(uint64_t &s) { return (double)(splitmix(s) >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1)

// trial j of iteration k
Trial script_trial(const Script &S, int k, int j)
{
    const ScriptIter &I = S.it[k];
    Trial T;
    if (I.nrej >= 0 && j > I.nrej) {   // behind the accepted one: the sequential search never evaluates it
        T.ea = T.ei = std::numeric_limits<double>::quiet_NaN();
        for (double &r : T.R) r = std::numeric_limits<double>::quiet_NaN();
        return T;
    }
    uint64_t s = S.seed ^ (0x1000003ull * (uint64_t)(k + 1)) ^ (0x10000000003ull * (uint64_t)(j + 1));
    for (double &r : T.R) r = 2.0 * unit(s) - 1.0;
    T.R[0] = S.tol * (2.0 + unit(s));
    T.R[1] = std::abs(T.R[1]) + 1e-3;
    if (j == I.nrej) {
        T.ea = I.ea;
        T.ei = I.ei;
        T.R[0] = I.g2;
        if (I.ysNeg) T.R[1] = (splitmix(s) & 1) ? 0.0 : -T.R[1];
    } else {   // rejected: above the iteration's starting energy by far more than the rounding of the two columns' sum
        T.ea = unit(s);
        T.ei = I.Eprev + (1e-3 + unit(s)) * (1.0 + std::abs(I.Eprev)) - S.dtSq * T.ea;
    }
    return T;
}

// kind: 0 random, 1 converges at the first iteration, 2 the cap falls into an iteration that halves, 3 collapses
Script make_script(uint64_t seed, int kind)
{
    std::mt19937_64 rng(seed);
    auto u = [&]() { return std::uniform_real_distribution<double>(0.0, 1.0)(rng); };
    Script S;
    S.seed = seed * 0x2545F4914F6CDD1Dull + 77;
    S.hist = 1 + (int)(seed % HIST_MAX);
    S.iterCap = 1 + (int)(rng() % 30);
    S.logCap = (rng() % 3 == 0) ? 4 : 64;
    S.tol = 1e-6;
    S.dtSq = 1e-4 * (1.0 + u());
    S.alphaMin = (rng() % 4 == 0) ? 0.25 : 0.1;
    S.ea0 = 10.0 * u();
    S.ei0 = u();
    S.g2_0 = 1.0 + u();
    int stopAt = 1 + (int)(rng() % 40);   // the iteration whose accepted trial meets the tolerance
    if (kind == 1) stopAt = 1, S.iterCap += 1;
    if (kind >= 2) stopAt = 1 << 20;
    const int collapseAt = (kind == 3) ? (int)(rng() % S.iterCap) : ((kind == 0 && rng() % 50 == 0) ? (int)(rng() % S.iterCap) : -1);
    double E = S.dtSq * S.ea0 + S.ei0;
    for (int k = 0; k < S.iterCap && k < stopAt; ++k) {
        ScriptIter I;
        I.Eprev = E;
        // alpha_0: the unit step (the quotient at or above 1), inside one of pair_band's three bands, or at the lower bound
        const int cls = (int)(rng() % 6);
        const double q = cls == 0 ? 1.0 : cls == 1 ? 1.0 + u() : cls == 2 ? 0.3 + 0.4 * u() : cls == 3 ? 0.7 + 0.2 * u() :
                         cls == 4 ? 0.9 + 0.09 * u() : 0.5 * S.alphaMin * u();
        I.pHp = 0.5 + u();
        I.pg = -q * I.pHp;
        I.nrej = (rng() % 2) ? 0 : 1 + (int)(rng() % 4);
        if (kind == 2 && k == S.iterCap - 1 && I.nrej == 0) I.nrej = 1 + (int)(rng() % 4);
        if (k == collapseAt) I.nrej = -1;
        I.ysNeg = rng() % 5 == 0;
        I.g2 = (k + 1 == stopAt) ? ((rng() % 4 == 0) ? S.tol : S.tol * u()) : S.tol * (2.0 + u());
        // accepted: at or below the starting energy -- one time in ten exactly at it (not an increase: accepted)
        const double target = (rng() % 10 == 0) ? E : E - 1e-2 * u() * (1.0 + std::abs(E));
        I.ea = 10.0 * u();
        I.ei = target - S.dtSq * I.ea;
        while (S.dtSq * I.ea + I.ei > E) I.ei = std::nextafter(I.ei, -std::numeric_limits<double>::infinity());
        S.it.push_back(I);
        if (I.nrej < 0) break;
        E = S.dtSq * I.ea + I.ei;
    }
    return S;
}

// ---- the sequential model ---------------------------------------------------------------------------------------------------
struct Accepted {   // the state an accepted trial leaves
    double alpha, E, g2;
    int m, order[HIST_MAX + 1], slot, status;
    double ys[HIST_MAX], b[HIST_MAX], sy[HIST_MAX][HIST_MAX], xi[HIST_MAX];
};
struct ModelRun {
    int iter = 0, halvings = 0, evals = 0, status = 0;
    double E_cur = 0, g2_cur = 0;
    std::vector<Accepted> acc;
};

// what must have occurred, counted over the model's runs ...
struct Classes {
    long a0One = 0, a0Band[3] = {0, 0, 0}, a0Min = 0, rej[5] = {0, 0, 0, 0, 0}, ysNonPos = 0, hist[HIST_MAX + 1] = {0};
    long capWhileHalving = 0, convergedAtFirst = 0, end[4] = {0, 0, 0, 0};
} g_cls;
// ... and per drive of the simulator
struct DriveEvents {
    long slots = 0, pairRedo = 0, pairRejected = 0, specKept = 0, specRedo = 0, pastKindCap = 0;
};

ModelRun run_model(const Script &S, bool count)
{
    ModelRun M;
    Accepted H;
    memset(&H, 0, sizeof(H));
    M.E_cur = S.dtSq * S.ea0 + S.ei0;
    M.g2_cur = S.g2_0;
    M.evals = 1;
    int slot = 0;
    if (count) g_cls.hist[S.hist]++;
    while (M.status == 0) {
        const int k = M.iter;
        double alpha = -S.it[k].pg / S.it[k].pHp;   // Optimizer.cpp:1085
        if (alpha > 1.0) alpha = 1.0;
        if (alpha < S.alphaMin) alpha = S.alphaMin;
        if (count) {
            if (alpha == 1.0) g_cls.a0One++;
            else g_cls.a0Band[alpha < 0.7 ? 0 : alpha < 0.9 ? 1 : 2]++;
            if (alpha == S.alphaMin) g_cls.a0Min++;
        }
        int j = 0;
        Trial T = script_trial(S, k, j);
        double E = S.dtSq * T.ea + T.ei;
        M.evals++;
        bool failed = false;
        while (E > M.E_cur && alpha > 0.0) {
            alpha /= 2.0;
            M.halvings++;
            if (alpha == 0.0) {
                failed = true;
                break;
            }
            T = script_trial(S, k, ++j);
            E = S.dtSq * T.ea + T.ei;
            M.evals++;
        }
        M.E_cur = E;
        if (failed) {
            M.status = 3;
            break;
        }
        if (count && j >= 1 && j <= 4) g_cls.rej[j]++;
        if (count && !(T.R[1] > 0.0)) g_cls.ysNonPos++;
        M.g2_cur = T.R[0];
        lbfgs_push_pair(S.hist, slot, T.R[1], T.R[2], T.R + 3, T.R + 3 + HIST_MAX, T.R + 3 + 2 * HIST_MAX, H.m, H.order, H.ys, H.b, H.sy);
        H.alpha = alpha;
        H.E = E;
        H.g2 = M.g2_cur;
        M.iter++;
        if (M.iter >= S.iterCap) M.status = 2;
        else if (!(M.g2_cur > S.tol)) M.status = 1;
        if (M.status == 0) {
            lbfgs_two_loop_xi(H.m, H.b, H.sy, H.ys, H.xi);
            slot = lbfgs_free_slot(S.hist, H.m, H.order);
        }
        H.slot = slot;
        H.status = M.status;
        M.acc.push_back(H);
        if (count && M.status == 2 && j >= 1) g_cls.capWhileHalving++;
        if (count && M.status == 1 && M.iter == 1) g_cls.convergedAtFirst++;
    }
    if (count) g_cls.end[M.status]++;
    return M;
}

// ---- the slot simulator -----------------------------------------------------------------------------------------------------
bool same(const void *a, const void *b, size_t n) { return memcmp(a, b, n) == 0; }

#define CHECK(cond, what)                                                                                                    \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "loopctl_check: form %d, script %llu, slot %d: %s\n", CTL, (unsigned long long)S.seed, C.slots, what); \
            return false;                                                                                                    \
        }                                                                                                                    \
    } while (0)

template <int CTL>
bool drive(const Script &S, const ModelRun &M, int pairCtr0, DriveEvents &ev)
{
    constexpr bool PAIR = CTL == CTL_PAIR || CTL == CTL_PAIR_VP, SPEC = CTL == CTL_SPEC;
    constexpr int KIND_CAP = 16;
    static double pool[4 * (HIST_MAX + 1)], xg[4];   // addresses only: nothing is read or written through them
    std::vector<double> logA(S.logCap), logE(S.logCap), logG(S.logCap);   // (exact extents: the sanitizer sees a write past the cap)
    std::vector<int> kinds(KIND_CAP, 0);
    DevLoop C;
    memset(&C, 0, sizeof(C));
    C.iterCap = S.iterCap;
    C.hist = S.hist;
    C.tol = S.tol;
    C.dtSq = S.dtSq;
    C.alphaMin = S.alphaMin;
    C.x_cur = xg, C.x_trial = xg + 1, C.g_cur = xg + 2, C.g_trial = xg + 3;
    for (int s = 0; s <= HIST_MAX; ++s) {
        C.S[s] = pool + 4 * s;
        C.Y[s] = pool + 4 * s + 1;
        C.MY[s] = pool + 4 * s + 2;
        C.HS[s] = pool + 4 * s + 3;
    }
    devloop_resolve(C);
    C.holdEnable = 1;
    for (int &c : C.pairCtr) c = pairCtr0;
    C.log_alpha = logA.data(), C.log_E = logE.data(), C.log_g2 = logG.data();
    C.slot_kind = kinds.data();
    C.logCap = S.logCap;
    C.kindCap = KIND_CAP;
    C.notifyFrom = 1 << 30;

    int published = 0, stops = 0, lastStopSlots = 0;
    bool verdictOk = true;
    auto recorder = [&](bool stop, int slots, int verdict) {
        published++;
        stops += stop ? 1 : 0;
        if (stop) lastStopSlots = slots;
        verdictOk = verdictOk && slots == C.slots && verdict == 2 * slots + (stop ? 1 : 0);
    };
    const double nan = std::numeric_limits<double>::quiet_NaN();
    {
        double R[RED_K + 2] = {0};
        R[0] = S.g2_0, R[RED_K] = S.ea0, R[RED_K + 1] = S.ei0;
        loop_verdict<CTL>(C, R, 1, nan, 0.0, 0.0, 0.0, 1.0, recorder);
        CHECK(published == 0 && C.evals == 1 && C.slots == 0 && C.status == 0, "the start-of-step evaluation decides something");
        const double E0 = S.dtSq * S.ea0 + S.ei0;
        CHECK(same(&C.E_cur, &E0, 8) && same(&C.E0, &E0, 8) && C.g2_0 == S.g2_0 && C.g2_cur == S.g2_0, "the start-of-step energy and |g|^2");
    }
    int j = 0, xSwaps = 0, gSwaps = 0;
    double a0 = 0.0, aj = 0.0;   // the running direction's alpha_0 and the step of trial j, halved here
    while (C.status == 0) {
        CHECK(C.slots < 100000, "the loop does not end");
        const int k = C.iter, phase = C.phase, iterBefore = C.iter, pubBefore = published;
        double *const xBefore = C.x_cur, *const gBefore = C.g_cur;
        double alpha_in, alpha_full = 0.0, ea = 0.0, ei = 0.0;
        Trial T;
        if (phase == 0) {
            a0 = ls_first_step(S.it[k].pg, S.it[k].pHp, S.alphaMin);
            // (the element kernels' rule, spelled out in k_elembody.hpp / k_elemvert.hip: behind a shared function their code changed)
            const bool paired = PAIR && a0 < 1.0 && a0 / 2.0 > 0.0 && C.pairCtr[pair_band(a0)] >= 3;
            j = paired ? 1 : 0;
            aj = paired ? a0 / 2.0 : a0;
            alpha_in = SPEC ? 1.0 : aj;
            T = script_trial(S, k, j);
            if (paired) {
                const Trial F = script_trial(S, k, 0);
                alpha_full = a0, ea = F.ea, ei = F.ei;
            }
            if (SPEC && a0 != 1.0) {   // the unit step is no trial of this search
                T.ea = T.ei = nan;
                for (double &r : T.R) r = nan;
            }
        } else {
            if ((PAIR || SPEC) && C.redo) j = 0, aj = a0;
            else j += 1, aj /= 2.0;
            alpha_in = C.alpha;
            CHECK(same(&alpha_in, &aj, 8), "a retry slot's step is not alpha_0 / 2^j");
            T = script_trial(S, k, j);
        }
        double R[RED_K + 2];
        memcpy(R, T.R, sizeof(T.R));
        R[RED_K] = T.ea, R[RED_K + 1] = T.ei;
        const int pairSlots = C.pairSlots, pairRedo = C.pairRedo, specSlots = C.specSlots, specRedo = C.specRedo;
        loop_verdict<CTL>(C, R, 0, alpha_in, alpha_full, ea, ei, a0, recorder);
        ev.slots++;
        // (c)
        CHECK(published == pubBefore + 1 && verdictOk, "a slot publishes once, holdVerdict = 2 slots + stop");
        CHECK(C.holdVerdict == 2 * C.slots + (lastStopSlots == C.slots ? 1 : 0) && C.abortEpoch == lastStopSlots, "the state's copy of the verdict");
        if (C.slots <= KIND_CAP) CHECK(kinds[C.slots - 1] == (phase == 0 ? 1 : 2), "slot_kind");
        else ev.pastKindCap++;
        ev.pairRedo += C.pairRedo - pairRedo;
        ev.pairRejected += (C.pairSlots - pairSlots) - (C.pairRedo - pairRedo);
        ev.specRedo += C.specRedo - specRedo;
        ev.specKept += (C.specSlots - specSlots) - (C.specRedo - specRedo);
        // (d)
        xSwaps += C.x_cur != xBefore;
        gSwaps += C.g_cur != gBefore;
        CHECK((C.x_cur == xBefore) == (C.x_trial != xBefore) && (C.g_cur == gBefore) == (C.g_trial != gBefore), "a swap loses a pointer");
        // (a), per accepted trial
        if (C.iter != iterBefore) {
            CHECK(C.iter == iterBefore + 1 && C.iter <= (int)M.acc.size(), "an accept the model does not have");
            const Accepted &A = M.acc[C.iter - 1];
            const int m = A.m;
            CHECK(same(&C.E_cur, &A.E, 8) && same(&C.g2_cur, &A.g2, 8) && C.status == A.status, "E_cur / g2_cur / status after an accept");
            CHECK(C.L.m == m && same(C.order, A.order, sizeof(int) * m) && same(C.L.ys, A.ys, 8 * m) && same(C.b, A.b, 8 * m), "m / order / ys / b");
            for (int i = 0; i < m; ++i) {
                CHECK(same(C.L.sy[i], A.sy[i], 8 * m), "sy");
                CHECK(C.L.s[i] == C.S[C.order[i]] && C.L.y[i] == C.Y[C.order[i]], "the chronological views");
            }
            if (C.status == 0) CHECK(same(C.X.xi, A.xi, sizeof(A.xi)) && C.slot == A.slot && C.phase == 0, "xi / free slot of the next direction");
            if (C.iter <= S.logCap)
                CHECK(same(&logA[C.iter - 1], &A.alpha, 8) && same(&logE[C.iter - 1], &A.E, 8) && same(&logG[C.iter - 1], &A.g2, 8), "the log");
        }
    }
    // (a), the step
    CHECK(C.iter == M.iter && C.halvings == M.halvings && C.evals == M.evals && C.status == M.status, "iter / halvings / evals / status");
    CHECK(same(&C.E_cur, &M.E_cur, 8) && same(&C.g2_cur, &M.g2_cur, 8), "E_cur / g2_cur at the end");
    // (b)
    CHECK(stops == loop_stopped_launches(C.halvings, C.pairSlots, C.pairRedo, C.specRedo) - (C.status == 3 ? 1 : 0), "the stopped-launch count");
    // (d)
    CHECK(xSwaps == M.iter + (M.status == 3 ? 1 : 0) && gSwaps == M.iter, "swaps of x / g");
    return true;
}

bool drive_form(int cfg, const Script &S, const ModelRun &M, DriveEvents &ev)
{
    switch (cfg) {
    case 0: return drive<CTL_PLAIN>(S, M, 1, ev);
    case 1: return drive<CTL_PAIR>(S, M, 1, ev);      // cold: the counters a fresh handle starts with
    case 2: return drive<CTL_PAIR>(S, M, 3, ev);      // saturated
    case 3: return drive<CTL_SPEC>(S, M, 1, ev);
    case 4: return drive<CTL_VP>(S, M, 1, ev);
    case 5: return drive<CTL_PAIR_VP>(S, M, 1, ev);
    default: return drive<CTL_PAIR_VP>(S, M, 3, ev);
    }
}
const char *const CFG_NAME[7] = {"PLAIN", "PAIR cold", "PAIR saturated", "SPEC", "VP", "PAIR_VP cold", "PAIR_VP saturated"};

// ---- (e) the controller's sums ------------------------------------------------------------------------------------------------
template <int STRIDE>
bool check_sums(std::mt19937_64 &rng)
{
    const int sizes[] = {1, 15, 16, 17, 100, 512, NB_RED};
    std::uniform_real_distribution<double> val(-1.0, 1.0);
    for (int n : sizes) {
        std::vector<double> p((size_t)n * STRIDE);   // (exact extent)
        for (double &v : p) v = val(rng);
        for (int c = 0; c < STRIDE; ++c) {
            double tot = 0.0;
            for (int ch = 0; ch < SUM_CHUNKS; ++ch) tot += ctl_chunk_sum<STRIDE>(p.data() + c, n, ch);
            const double ref = chunked_sum(n, [&](int k) { return p[(size_t)k * STRIDE + c]; });
            if (!same(&tot, &ref, 8)) {
                fprintf(stderr, "loopctl_check: ctl_chunk_sum<%d> differs from chunked_sum: n %d, column %d\n", STRIDE, n, c);
                return false;
            }
        }
    }
    return true;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20240911);
    if (!check_sums<2>(rng) || !check_sums<RED_K>(rng)) return 1;

    constexpr int NRANDOM = 400;
    DriveEvents ev[7];
    long scripts = 0;
    for (int n = 0; n < NRANDOM + 3 * HIST_MAX; ++n) {
        const int kind = n < NRANDOM ? 0 : 1 + (n - NRANDOM) % 3;   // behind the random ones: each designed end at every history length
        const Script S = make_script(1000 + (uint64_t)n, kind);
        const ModelRun M = run_model(S, true);
        for (int cfg = 0; cfg < 7; ++cfg)
            if (!drive_form(cfg, S, M, ev[cfg])) {
                fprintf(stderr, "loopctl_check: (%s)\n", CFG_NAME[cfg]);
                return 1;
            }
        ++scripts;
    }
    // every class of case occurred
    bool all = g_cls.a0One && g_cls.a0Band[0] && g_cls.a0Band[1] && g_cls.a0Band[2] && g_cls.a0Min && g_cls.rej[1] && g_cls.rej[2] &&
               g_cls.rej[3] && g_cls.rej[4] && g_cls.ysNonPos && g_cls.capWhileHalving && g_cls.convergedAtFirst && g_cls.end[1] &&
               g_cls.end[2] && g_cls.end[3];
    for (int h = 1; h <= HIST_MAX; ++h) all = all && g_cls.hist[h];
    for (int cfg = 0; cfg < 7; ++cfg) all = all && ev[cfg].pastKindCap;                 // (a collapse: ~1 080 slots)
    for (int cfg : {1, 2, 5, 6}) all = all && ev[cfg].pairRedo && ev[cfg].pairRejected;   // cold counters learn to pair within a step
    all = all && ev[3].specRedo && ev[3].specKept;
    printf("loopctl_check: %ld scripts x 7 drives; ends: %ld converged, %ld at the cap, %ld collapsed; alpha_0: %ld unit, %ld / %ld / %ld in the "
           "bands, %ld at the bound; rejections 1-4: %ld / %ld / %ld / %ld; y.s <= 0: %ld; cap while halving: %ld; converged at once: %ld\n",
           scripts, g_cls.end[1], g_cls.end[2], g_cls.end[3], g_cls.a0One, g_cls.a0Band[0], g_cls.a0Band[1], g_cls.a0Band[2], g_cls.a0Min,
           g_cls.rej[1], g_cls.rej[2], g_cls.rej[3], g_cls.rej[4], g_cls.ysNonPos, g_cls.capWhileHalving, g_cls.convergedAtFirst);
    for (int cfg = 0; cfg < 7; ++cfg)
        printf("loopctl_check: %-18s %ld slots, %ld past slot_kind's extent; paired %ld redone / %ld rejected; speculative %ld kept / %ld redone\n",
               CFG_NAME[cfg], ev[cfg].slots, ev[cfg].pastKindCap, ev[cfg].pairRedo, ev[cfg].pairRejected, ev[cfg].specKept, ev[cfg].specRedo);
    if (!all) {
        fprintf(stderr, "loopctl_check: a class of case did not occur\n");
        return 1;
    }
    printf("loopctl_check: every drive equal to the sequential model\n");
    return 0;
}
