// Prints what attention_plan.h (tokensgen_amd/csrc) decides for a table of shapes: host only, no GPU.  tests/test_host_cpu.py::test_attention_plan_table holds the
// expected lines.  Every case: 256 CUs, the knobs at their defaults (TG_ATTN_PP_MIN_WG 1024, TG_ATTN_FIXEDM 1, TG_ATTN_SPLIT 1) unless it names one.
//   forward: one line per launch — kernel (pp<PRESCALED,FIXEDM,LSE,RETRY,SPLIT>), grid, block, LDS bytes, the problem covered and its query rows first+count,
//            `wgs main_wgs/total_wgs`, `split split_first+nsplit`.  "plain": not prescaled, no bounds, no workspaces; "full": prescaled K, every segment with
//            k_norm2_max, a retry workspace, ample split floats.  nk = nq unless named.
//   refusals: the code and text of attn_fwd_refusal, or `ok`.
//   backward: the workspace layout in 4-byte words; the plan, one line per problem and one for the one-kernel launch if there is one.
#include <stdio.h>

#include "attention_plan.h"

namespace {

constexpr int N_CU = 256;
const AttnKnobs kDefault{1024, 1, 1};
constexpr long AMPLE = 1L << 40;

AttnFwdShape plain(int heads, int batch, int nq, int r_nq = 0, int nseg = 1) {
    AttnFwdShape s{};
    s.heads = heads; s.batch = batch; s.nq = nq; s.r_nq = r_nq; s.nseg = nseg; s.nk1 = nq;
    return s;
}
AttnFwdShape full(int heads, int batch, int nq, int r_nq = 0, int nseg = 1) {
    AttnFwdShape s = plain(heads, batch, nq, r_nq, nseg);
    s.prescaled = s.kn2_all = s.retry = true;
    s.split_floats = AMPLE;
    return s;
}

void show(const char* name, const AttnFwdShape& s, const AttnKnobs& kn = kDefault) {
    const AttnFwdPlan pl = attn_fwd_plan(s, kn, N_CU);
    const char* const cover[] = {"main", "rider", "both"};
    for (int i = 0; i < pl.n; ++i) {
        const AttnLaunch& l = pl.l[i];
        char kernel[32];
        switch (l.kernel) {
            case ATTN_K_FWD1: snprintf(kernel, sizeof(kernel), "fwd<1>"); break;
            case ATTN_K_FWD2: snprintf(kernel, sizeof(kernel), "fwd<2>"); break;
            case ATTN_K_COMBINE: snprintf(kernel, sizeof(kernel), "combine(%d)", l.fixedm); break;
            case ATTN_K_PP: snprintf(kernel, sizeof(kernel), "pp<%d,%d,%d,%d,%d>", l.pp & 1, (l.pp >> 1) & 1, (l.pp >> 2) & 1, (l.pp >> 3) & 1, (l.pp >> 4) & 1); break;
        }
        printf("%s: %s grid %u block %d lds %d %s rows %d+%d wgs %d/%d split %d+%d\n", name, kernel, l.grid, l.block, l.lds, cover[l.cover], l.row0, l.rows, l.main_wgs,
               l.total_wgs, l.split_first, l.nsplit);
    }
}

AttnFwdDims dims(int heads, int batch, int nq, int nk = 64, long vt_ld = 64) {
    AttnFwdDims d{};
    d.heads = heads; d.batch = batch; d.nq = nq; d.nseg = 1; d.seg[0] = AttnSegDims{nk, vt_ld};
    return d;
}
AttnFwdDims with_rider(AttnFwdDims d, int r_nq, int r_nseg = 1, int nk = 64, long vt_ld = 64) {
    d.rider = true; d.r_nq = r_nq; d.r_nseg = r_nseg; d.r_seg = AttnSegDims{nk, vt_ld};
    return d;
}
AttnFwdDims with_seg2(AttnFwdDims d, int nk = 64, long vt_ld = 64) { d.nseg = 2; d.seg[1] = AttnSegDims{nk, vt_ld}; return d; }
AttnFwdDims with_retry(AttnFwdDims d, long ints) { d.retry = true; d.retry_ints = ints; return d; }
AttnFwdDims with_nseg(AttnFwdDims d, int nseg) { d.nseg = nseg; return d; }
AttnFwdDims per_item(AttnFwdDims d) { d.per_item_scales = true; return d; }

void refusal(const char* name, AttnEntry e, const AttnFwdDims& d) {
    const AttnRefusal r = attn_fwd_refusal(e, d);
    if (r.err) printf("%s: error %d: %s\n", name, r.err, r.msg);
    else printf("%s: ok\n", name);
}

void layout(int nq, int nk, int heads, int batch) {
    const AttnBwdLayout L = attn_bwd_layout(nq, nk, heads, batch);
    printf("layout nq %d nk %d heads %d batch %d: seed %ld lse %ld d %ld cnt %ld ncnt %ld xmask %ld dq_part %ld total %ld\n", nq, nk, heads, batch, L.seed, L.lse, L.d, L.cnt,
           L.ncnt, L.xmask, L.dq_part, L.total);
}

void bwd(const char* name, int heads, int batch, int flags, AttnBwdShape a, const AttnBwdShape* b = nullptr) {
    const AttnBwdShape s[2] = {a, b ? *b : AttnBwdShape{}};
    const int count = b ? 2 : 1;
    const AttnBwdPlan pl = attn_bwd_plan(s, count, heads, batch, flags, N_CU);
    for (int i = 0; i < count; ++i) {
        const AttnBwdProblemPlan& p = pl.pr[i];
        printf("%s: problem %d: %s stats %ux%u wgs_k %u kparts %d dq %u join %u\n", name, i, p.one_kernel ? "one kernel" : "two launches", p.stats_x, p.stats_y, p.wgs_k,
               p.kparts, p.dq_grid, p.join_grid);
    }
    if (pl.main_i >= 0)
        printf("%s: fused grid %u block 512 lds %d main %d rider %d main_wgs %d\n", name, pl.fused_grid, attn_cfg::PP_LDS, pl.main_i, pl.rider_i, pl.fused_main_wgs);
}

}  // namespace

int main() {
    // ---- forward: the workload's shapes.  The To2V block (main + vip-query rider), the same main problem alone, the T2To stage, the training forward ----
    show("full 48x2 nq 17776 + rider 226", full(48, 2, 17776, 226));
    show("plain 48x2 nq 17776", plain(48, 2, 17776));
    show("full 48x2 nq 9442", full(48, 2, 9442));
    { AttnFwdShape s = plain(48, 2, 17776); s.lse = true; show("plain lse 48x2 nq 17776", s); }
    { AttnFwdShape s = full(48, 2, 17776); s.lse = true; s.split_floats = 0; show("full lse 48x2 nq 17776", s); }
    { AttnFwdShape s = plain(48, 2, 17776); s.lse = s.prescaled = true; show("prescaled lse, no retry 48x2 nq 17776", s); }
    // the shape of test_attention_ragged_tile_split_at_launch_scale; below both thresholds; the 256-row kernel
    show("plain 48x2 nq 6806 2 segments", plain(48, 2, 13 * 512 + 150, 0, 2));
    show("plain 2x2 nq 700", plain(2, 2, 700));
    show("plain 48x2 nq 2816", plain(48, 2, 2816));
    // ---- pp_min_wg: 1023 / 1024 workgroups of 512 rows; 1024 with a ragged tile whose full tiles are 1023; the tests' setting 1 ----
    show("plain 1x1 nq 523776 (1023 wgs)", plain(1, 1, 523776));
    show("plain 1x1 nq 524288 (1024 wgs)", plain(1, 1, 524288));
    show("plain 1x1 nq 523777 (1023 full + ragged)", plain(1, 1, 523777));
    show("plain 2x2 nq 700 pp_min 1", plain(2, 2, 700), AttnKnobs{1, 1, 1});
    // ---- wg256 at 1023 / 1024 ----
    show("plain 1x1 nq 261888 (wg256 1023)", plain(1, 1, 261888));
    show("plain 1x1 nq 262144 (wg256 1024)", plain(1, 1, 262144));
    // ---- the ragged tail: no round saved (13 either way); a rider present ----
    show("plain 48x2 nq 16996", plain(48, 2, 16996));
    show("plain 48x2 nq 17776 + rider 226", plain(48, 2, 17776, 226));
    // ---- the split remainder R: 0, 100 (not a multiple of 8), n_cu / 2, n_cu / 2 + 1; a launch of at most n_cu workgroups; R = 1; R beyond the main problem ----
    show("full 1x1 nq 524288 (R 0)", full(1, 1, 524288));
    show("full 1x1 nq 575488 (R 100)", full(1, 1, 575488));
    show("full 1x1 nq 589824 (R 128)", full(1, 1, 589824));
    show("full 1x1 nq 590336 (R 129)", full(1, 1, 590336));
    show("full 8x1 nq 8192 pp_min 1 (128 wgs)", full(8, 1, 8192), AttnKnobs{1, 1, 1});
    show("full 1x1 nq 131072 pp_min 1 (256 wgs)", full(1, 1, 131072), AttnKnobs{1, 1, 1});
    show("full 1x1 nq 131584 pp_min 1 (257 wgs)", full(1, 1, 131584), AttnKnobs{1, 1, 1});
    show("full 1x1 nq 512 + rider 132608 pp_min 1 (R 4 > 1)", full(1, 1, 512, 132608), AttnKnobs{1, 1, 1});
    // ---- what else takes the split away: one key tile, a workspace one float short, a log-sum-exp, the knob ----
    { AttnFwdShape s = full(1, 1, 589824); s.nk1 = 64; show("full 1x1 nq 589824 nk 64", s); }
    { AttnFwdShape s = full(1, 1, 589824); s.nk1 = 65; show("full 1x1 nq 589824 nk 65", s); }
    { AttnFwdShape s = full(1, 1, 589824); s.split_floats = 2 * 128 * attn_cfg::SPLIT_HALF_FLOATS; show("full 1x1 nq 589824 split floats 17039360", s); }
    { AttnFwdShape s = full(1, 1, 589824); s.split_floats = 2 * 128 * attn_cfg::SPLIT_HALF_FLOATS - 1; show("full 1x1 nq 589824 split floats 17039359", s); }
    { AttnFwdShape s = full(1, 1, 589824); s.lse = true; show("full lse 1x1 nq 589824", s); }
    show("full 48x2 nq 17776 + rider 226 split 0", full(48, 2, 17776, 226), AttnKnobs{1024, 1, 0});
    // ---- what takes the constant shift away: the knob, a segment without k_norm2_max, no retry workspace, K not prescaled ----
    show("full 48x2 nq 17776 + rider 226 fixedm 0", full(48, 2, 17776, 226), AttnKnobs{1024, 0, 1});
    { AttnFwdShape s = full(48, 2, 17776, 226); s.kn2_all = false; show("full 48x2 nq 17776 + rider 226, a segment without bound", s); }
    { AttnFwdShape s = full(48, 2, 17776, 226); s.retry = false; show("full 48x2 nq 17776 + rider 226, no retry", s); }
    { AttnFwdShape s = full(48, 2, 17776, 226); s.prescaled = false; show("full 48x2 nq 17776 + rider 226, not prescaled", s); }
    // ---- all five launches: a ragged tail behind a split launch ----
    show("full 48x4 nq 3172", full(48, 4, 3172));
    // ---- a rider without a ping-pong launch to ride on: two dispatches; the rider alone may reach the ping-pong kernel (and has no workspace there) ----
    show("plain 2x2 nq 700 + rider 226", plain(2, 2, 700, 226));
    show("full 48x2 nq 2816 + rider 17776", full(48, 2, 2816, 17776));

    // ---- refusals: one per message, on each side of its limit ----
    refusal("fwd nq 0", ATTN_FWD, dims(48, 2, 0));
    refusal("fwd nq 1", ATTN_FWD, dims(48, 2, 1));
    refusal("fwd nk1 0", ATTN_FWD, dims(48, 2, 64, 0));
    refusal("fwd heads 0", ATTN_FWD, dims(0, 2, 64));
    refusal("fwd batch 0", ATTN_FWD, dims(48, 0, 64));
    refusal("multi 1x1 nq 1 nk 1", ATTN_FWD_MULTI, dims(1, 1, 1, 1));
    refusal("multi heads 0", ATTN_FWD_MULTI, dims(0, 2, 64));
    refusal("multi batch 0", ATTN_FWD_MULTI, dims(48, 0, 64));
    refusal("multi nq 0", ATTN_FWD_MULTI, dims(48, 2, 0));
    refusal("multi nseg 0", ATTN_FWD_MULTI, with_nseg(dims(48, 2, 64), 0));
    refusal("multi nseg 2", ATTN_FWD_MULTI, with_seg2(dims(48, 2, 64)));
    refusal("multi nseg 3", ATTN_FWD_MULTI, with_nseg(with_seg2(dims(48, 2, 64)), 3));
    refusal("multi segment 1 nk 0", ATTN_FWD_MULTI, dims(48, 2, 64, 0));
    refusal("multi segment 2 nk 0", ATTN_FWD_MULTI, with_seg2(dims(48, 2, 64), 0));
    refusal("multi segment 1 nk 64 vt_ld 64", ATTN_FWD_MULTI, dims(48, 2, 64, 64, 64));
    refusal("multi segment 1 nk 65 vt_ld 64", ATTN_FWD_MULTI, dims(48, 2, 64, 65, 64));
    refusal("multi segment 1 nk 65 vt_ld 128", ATTN_FWD_MULTI, dims(48, 2, 64, 65, 128));
    refusal("multi segment 2 nk 65 vt_ld 64", ATTN_FWD_MULTI, with_seg2(dims(48, 2, 64), 65, 64));
    refusal("multi per-item scales batch 16", ATTN_FWD_MULTI, per_item(with_seg2(dims(48, 16, 64))));
    refusal("multi per-item scales batch 17", ATTN_FWD_MULTI, per_item(with_seg2(dims(48, 17, 64))));
    refusal("multi one scale batch 17", ATTN_FWD_MULTI, with_seg2(dims(48, 17, 64)));
    refusal("multi rider nq 1", ATTN_FWD_MULTI, with_rider(dims(48, 2, 64), 1));
    refusal("multi rider nq 0", ATTN_FWD_MULTI, with_rider(dims(48, 2, 64), 0));
    refusal("multi rider nseg 2", ATTN_FWD_MULTI, with_rider(dims(48, 2, 64), 64, 2));
    refusal("multi rider nk 0", ATTN_FWD_MULTI, with_rider(dims(48, 2, 64), 64, 1, 0));
    refusal("multi rider nk 65 vt_ld 64", ATTN_FWD_MULTI, with_rider(dims(48, 2, 64), 64, 1, 65, 64));
    refusal("multi 48x2 nq 17776 + rider 226 retry 3457", ATTN_FWD_MULTI, with_retry(with_rider(dims(48, 2, 17776), 226), 3457));
    refusal("multi 48x2 nq 17776 + rider 226 retry 3456", ATTN_FWD_MULTI, with_retry(with_rider(dims(48, 2, 17776), 226), 3456));
    refusal("lse nq 1", ATTN_FWD_LSE, dims(48, 2, 1));
    refusal("lse nq 0", ATTN_FWD_LSE, dims(48, 2, 0));
    refusal("lse nk 0", ATTN_FWD_LSE, dims(48, 2, 64, 0));
    refusal("lse nk 65 vt_ld 64", ATTN_FWD_LSE, dims(48, 2, 64, 65, 64));
    refusal("lse_ex heads 0", ATTN_FWD_LSE_EX, dims(0, 2, 64));
    refusal("lse_ex batch 0", ATTN_FWD_LSE_EX, dims(48, 0, 64));
    refusal("lse_ex 48x2 nq 17776 retry 3361", ATTN_FWD_LSE_EX, with_retry(dims(48, 2, 17776), 3361));
    refusal("lse_ex 48x2 nq 17776 retry 3360", ATTN_FWD_LSE_EX, with_retry(dims(48, 2, 17776), 3360));

    // ---- backward: the workspace layout of the workload's calls (main, vip-query), the smallest shape, odd sizes, the dQ partials on each side of 256 blocks ----
    layout(17776, 17776, 48, 2);
    layout(480, 18256, 48, 2);
    layout(1, 1, 1, 1);
    layout(33, 7, 3, 1);
    layout(65536, 64, 1, 1);
    layout(65537, 64, 1, 1);
    // ---- backward plans: the main call with and without the flag, dQ not 16-byte usable, heads * batch not a multiple of 8 ----
    const AttnBwdShape main_call{17776, 17776, true}, vip_query{480, 18256, true}, vip_key{17776, 480, true};
    bwd("48x2 17776x17776 flag", 48, 2, TG_BWD_ONE_KERNEL, main_call);
    bwd("48x2 17776x17776", 48, 2, 0, main_call);
    bwd("48x2 17776x17776 flag dq unaligned", 48, 2, TG_BWD_ONE_KERNEL, AttnBwdShape{17776, 17776, false});
    bwd("47x2 17776x17776 flag", 47, 2, TG_BWD_ONE_KERNEL, main_call);
    // query tiles at 4 * key blocks - 1 / 4 * key blocks (70 key blocks)
    bwd("48x2 8928x17776 flag (279 tiles)", 48, 2, TG_BWD_ONE_KERNEL, AttnBwdShape{8928, 17776, true});
    bwd("48x2 8929x17776 flag (280 tiles)", 48, 2, TG_BWD_ONE_KERNEL, AttnBwdShape{8929, 17776, true});
    // the dQ split: the vip-query call; dQ not 16-byte usable; query blocks at 256 / 257; key tiles / 16 clamping kparts, and taking it to 1
    bwd("48x2 480x18256 flag", 48, 2, TG_BWD_ONE_KERNEL, vip_query);
    bwd("48x2 480x18256 dq unaligned", 48, 2, 0, AttnBwdShape{480, 18256, false});
    bwd("32x8 256x4096 (256 blocks)", 32, 8, 0, AttnBwdShape{256, 4096, true});
    bwd("257x1 256x4096 (257 blocks)", 257, 1, 0, AttnBwdShape{256, 4096, true});
    bwd("48x2 480x1536 (48 key tiles)", 48, 2, 0, AttnBwdShape{480, 1536, true});
    bwd("48x2 480x992 (31 key tiles)", 48, 2, 0, AttnBwdShape{480, 992, true});
    // two problems: both, one (in either order), neither in the one-kernel form
    bwd("48x2 main + vip-key flag", 48, 2, TG_BWD_ONE_KERNEL, main_call, &vip_key);
    bwd("48x2 main + vip-query flag", 48, 2, TG_BWD_ONE_KERNEL, main_call, &vip_query);
    bwd("48x2 vip-query + main flag", 48, 2, TG_BWD_ONE_KERNEL, vip_query, &main_call);
    bwd("48x2 main + vip-key", 48, 2, 0, main_call, &vip_key);
    return 0;
}
