// What the attention entry points of attention.hip and attention_bwd.hip launch for a shape — kernels, grids, blocks, LDS bytes, the sub-problem each launch
// covers — which shapes the forward refuses, and where everything lies in the backward's workspace: pure host functions.  No HIP, no globals, no knob or
// device reads: the entry points pass the live knobs and the CU count in, a CPU test (tests/csrc/attention_plan_table.cpp) passes its own.
#pragma once
#include <stdio.h>

#include "tg_errors.h"
#include "tokensgen_hip.h"      // TG_BWD_ONE_KERNEL (plain C declarations only)

// ---- sizes that the kernels and their launches share ----
namespace attn_cfg {
constexpr int KVBLK = 64;                  // keys per tile
constexpr int TILE_B = 64 * 128;           // one 64x64 bf16 tile
constexpr int PP_ROWS = 512;               // query rows of one ping-pong workgroup
constexpr int PP_LDS_BYTES = 4 * TILE_B + 8 * 8192;         // attn_fwd_pp_kernel: 96 KiB of dynamic LDS
constexpr long SPLIT_HALF_FLOATS = 512L * (64 + 2 + 64);     // per half: O [512][64], m [512], l [512], O2 [512][64] (second half of a 2-segment parent)
// the retry workspace: retry[0] counts the re-run workgroups, retry[RETRY_FLAGS + wgid] is workgroup wgid's flag
constexpr int RETRY_FLAGS = 1;
// backward
constexpr int HEAD_DIM = 64;
constexpr int BT = 32;                     // rows of the streamed tile
constexpr int LQ2 = 72;                    // [row][d] tile: row stride in elements (144 B)
constexpr int ROWT_EL = BT * LQ2;
constexpr int DSLD = 40;                   // dS^T tile row stride in elements (80 B: 8-byte aligned 4-query runs)
constexpr int DQLD = 68;                   // dQ tile row stride in floats (272 B: the 16 lanes of a block column land on different banks)
constexpr int PP_RING = 4;
constexpr int PP_ST_BYTES = 2 * PP_RING * ROWT_EL * 2;          // Q | dO tiles
constexpr int PP_SEED_BYTES = PP_RING * 64 * 16;
constexpr int PP_DS_SLOT = 256 * DSLD * 2;                      // one dS^T tile [256 keys][DSLD] bf16
constexpr int PP_DQ_SLOT = BT * DQLD * 4;                       // one dQ partial [32 q][DQLD] fp32
constexpr int PP_LDS = PP_ST_BYTES + PP_SEED_BYTES + 2 * PP_DS_SLOT + 4 * PP_DQ_SLOT;      // attn_bwd_fused_pp_kernel
constexpr int DQ_SPLIT_MAX = 8;            // key ranges of the dQ launch at most
}  // namespace attn_cfg

// =================================================================== forward ===================================================================

// workgroups of 512 query rows: of one problem, and of a launch (the rider's follow the main problem's; r_nq 0: no rider)
inline long attn_wg512(int nq, int heads, int batch) { return (long)((nq + attn_cfg::PP_ROWS - 1) / attn_cfg::PP_ROWS) * heads * batch; }
inline long attn_grid512(int nq, int r_nq, int heads, int batch) { return attn_wg512(nq, heads, batch) + (r_nq > 0 ? attn_wg512(r_nq, heads, batch) : 0); }
inline long attn_retry_ints(int nq, int r_nq, int heads, int batch) { return attn_cfg::RETRY_FLAGS + attn_grid512(nq, r_nq, heads, batch); }
// The half-round rule: when the last round of a launch of grid512 workgroups fills at most half of the CUs, its R workgroups are split over the key axis
// (0: no split).
inline long attn_split_remainder(long grid512, int n_cu) {
    const long R = grid512 % n_cu;
    return (grid512 > n_cu && 2 * R <= n_cu) ? R : 0;
}
inline long attn_split_floats(long R) { return 2 * R * attn_cfg::SPLIT_HALF_FLOATS; }

struct AttnKnobs { long pp_min_wg; int fixedm, split; };      // TG_ATTN_PP_MIN_WG, TG_ATTN_FIXEDM, TG_ATTN_SPLIT

struct AttnFwdShape {
    int nq, r_nq;                // r_nq 0: no rider
    int heads, batch, nseg;
    int nk1;                     // main segment 1's keys
    bool prescaled, lse;
    bool kn2_all;                // every segment, the rider's included, carries k_norm2_max
    bool retry;                  // a retry workspace was given
    long split_floats;           // floats of split workspace given (0: none)
};

enum AttnKernel { ATTN_K_FWD1, ATTN_K_FWD2, ATTN_K_PP, ATTN_K_COMBINE };       // attn_fwd_kernel<1>, <2>, attn_fwd_pp_kernel<...>, attn_split_combine_kernel
enum AttnCover { ATTN_MAIN, ATTN_RIDER, ATTN_BOTH };                          // the main problem without its rider, the rider as a problem of its own, both

// attn_fwd_pp_kernel<PRESCALED, FIXEDM, LSE, RETRY, SPLIT> as one number
constexpr int attn_pp_id(bool prescaled, int fixedm, bool lse, bool retry, bool split) {
    return (prescaled ? 1 : 0) | (fixedm ? 2 : 0) | (lse ? 4 : 0) | (retry ? 8 : 0) | (split ? 16 : 0);
}

struct AttnLaunch {
    AttnKernel kernel;
    int pp;                      // ATTN_K_PP: attn_pp_id of the instantiation
    int fixedm;                  // ATTN_K_COMBINE: its fixedm argument
    unsigned grid;
    int block, lds;
    AttnCover cover;
    int row0, rows;              // the query rows of the covered main (ATTN_RIDER: rider) problem that this launch works on
    int main_wgs, total_wgs, split_first, nsplit;      // the AttnParams fields of the same names (per launch: a rider on its own is its own main problem)
};

struct AttnFwdPlan {
    int n;
    AttnLaunch l[5];             // at most: main, split halves, combine, retry, ragged tail
};

// one dispatch: a problem (with or without rider) whose rider, if any, has the ping-pong kernel to ride on
inline void attn_fwd_dispatch(AttnFwdPlan& pl, const AttnFwdShape& s, AttnCover cover, const AttnKnobs& kn, int n_cu) {
    using namespace attn_cfg;
    const int heads = s.heads, batch = s.batch;
    // kernel choice by query-range length: the 8-wave ping-pong kernel from `pp_min_wg` workgroups of 512 rows (4 per CU) on; below that the
    // 4-wave kernel with 256-row tiles (2 query blocks per wave) while those still give >= 4 workgroups per CU, else 128-row tiles.
    // Measured on MI355X at N = 17776: ping-pong 1.12-1.18 PFLOP/s, 256-row tiles 0.90, 128-row tiles 0.85.
    const long wg256 = (long)((s.nq + 255) / 256) * heads * batch;
    const long wg_all = attn_wg512(s.nq, heads, batch);
    const bool pp = wg_all >= kn.pp_min_wg;
    // ---- ragged last query tile: every ping-pong workgroup takes the same time, so a launch of G workgroups costs ceil(G / CUs) rounds.
    // When dropping the ragged last tile of every (head, batch) saves a round, those rows go to the 4-wave kernel in 128-row workgroups
    // right behind the ping-pong launch (same stream): N = 17776 without a rider 7.69 -> 7.53 ms, the T2To stage's N = 9442 (19 -> 18
    // tiles: 8 -> 7 rounds).  With a rider problem the riders already fill the last round, and the split loses (measured 8.0 vs 7.75 ms).
    const int full_rows = (s.nq / PP_ROWS) * PP_ROWS;
    const long wg_full = (long)(s.nq / PP_ROWS) * heads * batch;
    const bool ragged = pp && s.r_nq == 0 && full_rows < s.nq && wg_full >= kn.pp_min_wg && (wg_full + n_cu - 1) / n_cu < (wg_all + n_cu - 1) / n_cu;
    const int nq = ragged ? full_rows : s.nq;                 // the rows of every launch but the tail's
    const long wg512 = ragged ? wg_full : wg_all;
    // constant-shift softmax (attn_fwd_pp_kernel<.., FIXEDM = 1>): every segment of a k_prescaled launch carries the key-norm bound and the
    // caller gave a retry workspace.  The TG_ATTN_FIXEDM knob = 0 (tg_debug_set) forces the running-max kernel.
    const bool fixedm = kn.fixedm != 0 && s.prescaled && pp && s.retry && s.kn2_all;
    const long grid512 = wg512 + (s.r_nq > 0 ? attn_wg512(s.r_nq, heads, batch) : 0);
    const unsigned retry_grid = (unsigned)(grid512 < n_cu ? grid512 : n_cu);
    // ---- last-round quantisation: every 512-row workgroup of a launch takes the same time (same key length), so G workgroups cost
    // ceil(G / CUs) rounds — the DiT's 3360 + 96 = 13.5 x 256 pay for 14.  When the remainder R = G mod CUs is at most half a round, R
    // workgroups are split over the KEY axis into 2 R half-length workgroups (their own launch behind the G - R whole ones, partials joined by
    // attn_split_combine_kernel): the tail then costs half a round, 13.5 instead of 14.  Splitting over the queries cannot do that (DESIGN §8:
    // 128-row workgroups are themselves badly quantised).  The split parents are the last R workgroups of the MAIN problem, not the riders:
    // the halves of one head's query tiles share that head's K / V in their XCD's L2, whereas every rider has a (batch, head) of its own and
    // 256 of those streaming at once are HBM-bound.  The TG_ATTN_SPLIT knob = 0 disables; needs the caller's split workspace.
    int nsplit = 0, split_first = (int)grid512;
    if (pp && kn.split != 0 && !s.lse) {
        const long R = attn_split_remainder(grid512, n_cu);
        const int nt_main = (s.nk1 + KVBLK - 1) / KVBLK;
        if (R > 0 && R <= wg512 && nt_main >= 2 && s.split_floats >= attn_split_floats(R)) {
            nsplit = (int)R;
            split_first = (int)(wg512 - R);
        }
    }
    AttnLaunch base{};
    base.cover = cover; base.row0 = 0; base.rows = nq;
    base.main_wgs = (int)wg512; base.total_wgs = (int)grid512; base.split_first = split_first; base.nsplit = nsplit;
    auto add = [&](AttnKernel kernel, unsigned grid, int block, int lds) -> AttnLaunch& {
        AttnLaunch& l = pl.l[pl.n++];
        l = base;
        l.kernel = kernel; l.grid = grid; l.block = block; l.lds = lds;
        return l;
    };
    auto add_pp = [&](unsigned grid, int id) { add(ATTN_K_PP, grid, 512, PP_LDS_BYTES).pp = id; };
    // whole workgroups | halves of the split parents (rounded up to whole groups of 16 = 8 XCDs x 2 halves) | the join, 4 workgroups per parent
    const unsigned main_grid = (unsigned)(grid512 - nsplit), split_grid = (unsigned)(16 * ((nsplit + 7) / 8)), combine_grid = (unsigned)(4 * nsplit);
    if (fixedm) {
        // the verified constant-shift pass, [the split tail and its join,] then the retry launch: a persistent grid that re-runs the flagged
        // workgroups (normally none)
        add_pp(main_grid, attn_pp_id(true, 1, s.lse, false, false));
        if (nsplit) {
            add_pp(split_grid, attn_pp_id(true, 1, false, false, true));
            add(ATTN_K_COMBINE, combine_grid, 256, 0).fixedm = 1;
        }
        add_pp(retry_grid, attn_pp_id(true, 0, s.lse, true, false));
    } else if (pp) {
        // (the running-max LSE kernel has one instantiation: it multiplies by scale_log2, which is 1 for prescaled K)
        const bool prescaled = s.prescaled && !s.lse;
        add_pp(main_grid, attn_pp_id(prescaled, 0, s.lse, false, false));
        if (nsplit) {
            add_pp(split_grid, attn_pp_id(prescaled, 0, false, false, true));
            add(ATTN_K_COMBINE, combine_grid, 256, 0).fixedm = 0;
        }
    } else if (wg256 >= 1024) {
        add(ATTN_K_FWD2, (unsigned)wg256, 256, 0);
    } else {
        add(ATTN_K_FWD1, (unsigned)((nq + 127) / 128 * heads * batch), 256, 0);
    }
    if (ragged) {                                             // the ragged remainder: 128-row workgroups of the 4-wave kernel
        base = AttnLaunch{};
        base.cover = cover; base.row0 = full_rows; base.rows = s.nq - full_rows;
        add(ATTN_K_FWD1, (unsigned)((base.rows + 127) / 128 * heads * batch), 256, 0);
    }
}

inline AttnFwdPlan attn_fwd_plan(const AttnFwdShape& s, const AttnKnobs& kn, int n_cu) {
    AttnFwdPlan pl{};
    if (s.r_nq > 0 && attn_wg512(s.nq, s.heads, s.batch) < kn.pp_min_wg) {
        // the rider needs the ping-pong kernel to ride on: without it, two dispatches — the main problem alone, then the rider as a plain
        // single-segment problem of its own (no workspaces, no log-sum-exp)
        AttnFwdShape m = s;
        m.r_nq = 0;
        attn_fwd_dispatch(pl, m, ATTN_MAIN, kn, n_cu);
        AttnFwdShape r{};
        r.nq = s.r_nq; r.heads = s.heads; r.batch = s.batch; r.nseg = 1; r.prescaled = s.prescaled;
        attn_fwd_dispatch(pl, r, ATTN_RIDER, kn, n_cu);
    } else {
        attn_fwd_dispatch(pl, s, s.r_nq > 0 ? ATTN_BOTH : ATTN_MAIN, kn, n_cu);
    }
    return pl;
}

// ---- the shapes the forward entry points refuse (pointer and alignment checks stay with the entry points) ----
enum AttnEntry { ATTN_FWD, ATTN_FWD_MULTI, ATTN_FWD_LSE, ATTN_FWD_LSE_EX };
struct AttnSegDims { int nk; long vt_ld; };
struct AttnFwdDims {
    int nq, heads, batch, nseg;
    AttnSegDims seg[2];
    bool rider;                  // a second problem is present
    int r_nq, r_nseg;
    AttnSegDims r_seg;
    bool per_item_scales;        // seg2_scale_batch given
    bool retry;                  // a retry workspace of retry_ints ints given
    long retry_ints;
};
struct AttnRefusal {
    int err;                     // TG_OK, or the code of a refused shape with its text in msg
    char msg[256];
};

#define ATTN_PLAN_REQUIRE(cond, code, ...)                 \
    do {                                                   \
        if (!(cond)) {                                     \
            r.err = (code);                                \
            snprintf(r.msg, sizeof(r.msg), __VA_ARGS__);   \
            return r;                                      \
        }                                                  \
    } while (0)

inline const char* attn_entry_name(AttnEntry e) {
    return e == ATTN_FWD ? "tg_attention_fwd" : e == ATTN_FWD_MULTI ? "tg_attention_fwd_multi" : e == ATTN_FWD_LSE ? "tg_attention_fwd_lse" : "tg_attention_fwd_lse_ex";
}
// what the entry points call a key segment in their texts
inline const char* attn_seg_name(AttnEntry e, bool rider, int sg) {
    return e != ATTN_FWD_MULTI ? "segment" : rider ? "problem 1" : sg == 0 ? "problem 0 segment 1" : "problem 0 segment 2";
}

inline AttnRefusal attn_fwd_refusal(AttnEntry e, const AttnFwdDims& d) {
    AttnRefusal r{};
    const char* who = attn_entry_name(e);
    if (e == ATTN_FWD) {         // the rest is tg_attention_fwd_multi's, which it forwards to
        ATTN_PLAN_REQUIRE(d.nq > 0 && d.seg[0].nk > 0 && d.heads > 0 && d.batch > 0, TG_ERR_SHAPE, "%s: bad shape nq=%d nk1=%d", who, d.nq, d.seg[0].nk);
        return r;
    }
    if (e == ATTN_FWD_MULTI) {
        ATTN_PLAN_REQUIRE(d.heads > 0 && d.batch > 0, TG_ERR_SHAPE, "%s: bad shape", who);
        ATTN_PLAN_REQUIRE(d.nq > 0 && (d.nseg == 1 || d.nseg == 2), TG_ERR_ARG, "%s: problem 0", who);
    } else {
        ATTN_PLAN_REQUIRE(d.nq > 0 && d.seg[0].nk > 0 && d.heads > 0 && d.batch > 0, TG_ERR_SHAPE, "%s: bad shape nq=%d nk=%d", who, d.nq, d.seg[0].nk);
    }
    auto seg = [&](const AttnSegDims& g, const char* what) {
        ATTN_PLAN_REQUIRE(g.nk > 0, TG_ERR_SHAPE, "tg_attention: %s: nk=%d", what, g.nk);
        ATTN_PLAN_REQUIRE(g.vt_ld >= ((g.nk + 63) / 64) * 64, TG_ERR_SHAPE, "tg_attention: %s: vt_ld must cover nk rounded up to 64", what);
        return r;
    };
    for (int sg = 0; sg < d.nseg; ++sg)
        if (seg(d.seg[sg], attn_seg_name(e, false, sg)).err) return r;
    ATTN_PLAN_REQUIRE(!d.per_item_scales || d.batch <= 16, TG_ERR_SHAPE, "%s: per-item segment-2 scales for at most 16 batch items (got %d)", who, d.batch);
    if (d.rider) {
        ATTN_PLAN_REQUIRE(d.r_nq > 0 && d.r_nseg == 1, TG_ERR_ARG, "%s: problem 1 must have one key segment", who);
        if (seg(d.r_seg, attn_seg_name(e, true, 0)).err) return r;
    }
    if (d.retry) {
        const long need = attn_retry_ints(d.nq, d.rider ? d.r_nq : 0, d.heads, d.batch);
        ATTN_PLAN_REQUIRE(d.retry_ints >= need, TG_ERR_SHAPE, "%s: retry workspace of %ld ints, need %ld (tg_attention_retry_ints)", who, d.retry_ints, need);
    }
    return r;
}
#undef ATTN_PLAN_REQUIRE

// =================================================================== backward ===================================================================

// Every offset into a problem's workspace `ws`, in 4-byte words (floats and ints alike) from a 16-byte aligned base.
struct AttnBwdLayout {
    long seed;                   // the dK/dV kernel's seed rows, 16 B per query row (first: alignment)
    long lse, d;                 // per query row: log-sum-exp (unless the forward kept it), D
    long cnt, ncnt;              // the one-kernel form's exchange counters: offset (16-byte aligned) and count
    long xmask;                  // its per-head XCD masks, heads * batch ints behind the counters
    long dq_part;                // the dQ launch's key-range partials (few queries only), 16-byte aligned
    long total;                  // what tg_attention_bwd_ws_floats answers
};

// key-axis split of the dQ launch: only for calls with so few query blocks that one workgroup per block leaves most of the chip idle
inline bool attn_dq_split_shape(int nq, int heads, int batch) { return (long)((nq + 255) / 256) * heads * batch <= 256; }

inline AttnBwdLayout attn_bwd_layout(int nq, int nk, int heads, int batch) {
    using namespace attn_cfg;
    (void)nk;
    const long nhb = (long)batch * heads, nrow = nhb * nq;
    const long stats = 6 * nrow + 8;                           // 4 + 1 + 1 words per query row, and slack
    const long dq_floats = attn_dq_split_shape(nq, heads, batch) ? (long)DQ_SPLIT_MAX * batch * nq * heads * HEAD_DIM + 4 : 0;
    AttnBwdLayout L{};
    L.seed = 0;
    L.lse = 4 * nrow;
    L.d = 5 * nrow;
    L.cnt = (stats + 3) & ~3L;
    L.ncnt = nhb * ((nq + BT - 1) / BT) * 32;
    L.xmask = L.cnt + L.ncnt;
    L.dq_part = (L.xmask + nhb + 3) & ~3L;
    L.total = stats + L.ncnt + 8 + nhb + dq_floats;
    return L;
}

struct AttnBwdShape {
    int nq, nk;
    bool dq16;                   // dQ usable in 16-byte units: dq_ld % 4 == 0, dq_sb % 4 == 0, 16-byte aligned dq
};
struct AttnBwdProblemPlan {
    bool one_kernel;             // the form: one kernel (it joins the fused launch) / two launches (dK/dV, then dQ [and its join])
    unsigned stats_x, stats_y;   // attn_bwd_stats2_kernel: a 2-D grid, block 256
    unsigned wgs_k;              // key-block workgroups: attn_bwd_dkdv7_kernel's grid (block 512), or this problem's share of the fused launch
    int kparts;                  // key ranges of the dQ launch
    unsigned dq_grid, join_grid; // attn_bwd_dq2_kernel, attn_bwd_dq_join_kernel (block 256; join_grid 0: no join)
};
struct AttnBwdPlan {
    AttnBwdProblemPlan pr[2];
    int main_i, rider_i;         // the one-kernel problems: the first is the main call, a second one rides in the same launch (-1: none)
    unsigned fused_grid;         // attn_bwd_fused_pp_kernel: block 512, attn_cfg::PP_LDS bytes of dynamic LDS
    int fused_main_wgs;
};

inline AttnBwdPlan attn_bwd_plan(const AttnBwdShape* s, int count, int heads, int batch, int flags, int n_cu) {
    using namespace attn_cfg;
    AttnBwdPlan pl{};
    pl.main_i = pl.rider_i = -1;
    for (int i = 0; i < count; ++i) {
        AttnBwdProblemPlan& p = pl.pr[i];
        const int nq = s[i].nq, nk = s[i].nk;
        const unsigned gk_x = (unsigned)((nk + 255) / 256);
        p.stats_x = (unsigned)((nq + 255) / 256);
        p.stats_y = (unsigned)(batch * heads);
        p.wgs_k = gk_x * (unsigned)(batch * heads);
        // the ordered dQ accumulation runs the key blocks of a head as a chain a few tiles apart: worth it only when there are many more query tiles than
        // key blocks (the 17776^2 call: 556 tiles, 70 blocks; the vip queries' call with 15 tiles and 72 blocks would serialise)
        const bool chain_ok = (long)((nq + BT - 1) / BT) >= 4L * gk_x && s[i].dq16;
        p.one_kernel = (flags & TG_BWD_ONE_KERNEL) && chain_ok && ((heads * batch) & 7) == 0;
        p.kparts = 1;
        if (p.one_kernel) {
            if (pl.main_i < 0) {
                pl.main_i = i;
                pl.fused_main_wgs = (int)p.wgs_k;
            } else {
                pl.rider_i = i;
            }
            pl.fused_grid += p.wgs_k;
            continue;
        }
        // dQ: one workgroup per 256 queries and head — or, with few queries, per (256 queries, head, key range): ~3 rounds of the chip's resident slots (2 per CU)
        const long wgs = (long)p.stats_x * p.stats_y, ntile = (nk + BT - 1) / BT;
        if (attn_dq_split_shape(nq, heads, batch) && s[i].dq16) {
            p.kparts = (int)((6L * n_cu) / wgs);
            if (p.kparts > DQ_SPLIT_MAX) p.kparts = DQ_SPLIT_MAX;
            if (p.kparts > ntile / 16) p.kparts = (int)(ntile / 16);               // at least 16 key tiles per range
            if (p.kparts < 2) p.kparts = 1;
        }
        p.dq_grid = (unsigned)(wgs * p.kparts);
        if (p.kparts > 1) p.join_grid = (unsigned)(((long)batch * nq * heads * HEAD_DIM / 4 + 255) / 256);
    }
    return pl;
}
