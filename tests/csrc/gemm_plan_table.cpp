// Prints what gemm_plan() (tokensgen_amd/csrc/gemm_plan.h) decides for a table of shapes, one line per case: host only, no GPU.
// tests/test_host_cpu.py::test_gemm_plan_table holds the expected lines.  Every case: 256 CUs; unless it says otherwise batch 1, lda = ldw = K, ldt = ldb = R,
// vt_ld = M rounded up to 64, TG_GEMM_W4 = 1, the bias epilogue.  A case is named M x K -> N.
#include <stdio.h>

#include "gemm_plan.h"

namespace {

constexpr int N_CU = 256;
constexpr long LD_LIMIT = 1L << 21;
const char* const kKernelName[] = {"k128", "k256w8", "k256w4"};

void show(const char* name, const GemmShape& s, int w4 = 1) {
    const GemmPlan pl = gemm_plan(s, w4, N_CU);
    if (pl.err != TG_OK) {
        printf("%s: error %d: %s\n", name, pl.err, pl.msg);
        return;
    }
    printf("%s: %s grid %u block %d lds %d group_m %d\n", name, kKernelName[pl.kernel], pl.grid, pl.block, pl.lds, pl.group_m);
}

long pad64(long m) { return (m + 63) / 64 * 64; }

GemmShape plain(int M, int K, int N, int epilogue = TG_EPI_BIAS, int batch = 1) {
    GemmShape s{};
    s.entry = GEMM_PLAIN; s.M = M; s.N = N; s.K = K; s.batch = batch; s.epilogue = epilogue; s.lda = s.ldw = K;
    return s;
}
GemmShape pair(int M, int M2, int K, int N, int epilogue = TG_EPI_BIAS) {
    GemmShape s = plain(M, K, N, epilogue);
    s.entry = GEMM_PAIR; s.M2 = M2; s.second = true;
    return s;
}
GemmShape qkv(int M, int M2, int K, int N, int v_col0) {      // M2 == 0: one problem
    GemmShape s = plain(M, K, N);
    s.entry = GEMM_QKV; s.M2 = M2; s.second = M2 != 0; s.v_col0 = v_col0; s.vt_ld1 = pad64(M); s.vt_ld2 = pad64(M2);
    return s;
}
GemmShape lora(int M, int K, int N, int R) {
    GemmShape s = plain(M, K, N);
    s.entry = GEMM_LORA; s.R = R; s.ldt = s.ldb = R;
    return s;
}
GemmShape with_ld(GemmShape s, long lda, long ldw) { s.lda = lda; s.ldw = ldw; return s; }

}  // namespace

int main() {
    // the DiT block projections of the real workload (QKV and FF2), then K on each side of the group_m threshold
    show("plain 28326x3072->9216", plain(28326, 3072, 9216));
    show("plain 28326x12288->3072", plain(28326, 12288, 3072));
    show("plain 1024x8128->256", plain(1024, 8128, 256));
    show("plain 1024x8192->256", plain(1024, 8192, 256));
    // the 256x256 condition: M at 1023 / 1024, N a multiple of 128 only
    show("plain 1023x256->256", plain(1023, 256, 256));
    show("plain 1024x256->256", plain(1024, 256, 256));
    show("plain 1024x256->384", plain(1024, 256, 384));
    // the 4-wave condition: K at 192 / 256, the knob, the leading dimensions on each side of 2^21
    show("plain 1024x192->256", plain(1024, 192, 256));
    show("plain 1024x256->256 w4=0", plain(1024, 256, 256), 0);
    show("plain 1024x256->256 lda 2^21-8", with_ld(plain(1024, 256, 256), LD_LIMIT - 8, 256));
    show("plain 1024x256->256 lda 2^21", with_ld(plain(1024, 256, 256), LD_LIMIT, 256));
    show("plain 1024x256->256 ldw 2^21", with_ld(plain(1024, 256, 256), 256, LD_LIMIT));
    show("plain 2048x256->512 batch 2", plain(2048, 256, 512, TG_EPI_BIAS, 2));
    // the grid cap: tiles at n_cu - 1, n_cu, n_cu + 1
    show("plain 65280x256->256 (255 tiles)", plain(65280, 256, 256));
    show("plain 65536x256->256 (256 tiles)", plain(65536, 256, 256));
    show("plain 65537x256->256 (257 tiles)", plain(65537, 256, 256));
    // the 128x128 kernel: one grid entry per tile, no cap
    show("plain 1x512->18432", plain(1, 512, 18432));
    show("plain 300x64->128 batch 3", plain(300, 64, 128, TG_EPI_BIAS, 3));
    // the other epilogues
    show("plain gate_res 1024x256->256", plain(1024, 256, 256, TG_EPI_BIAS_GATE_RES));
    show("plain gate_res 1000x256->256", plain(1000, 256, 256, TG_EPI_BIAS_GATE_RES));
    show("plain keep_gelu 1024x256->256", plain(1024, 256, 256, TG_EPI_BIAS_KEEP_GELU));
    show("plain gelu_grad 1024x256->256", plain(1024, 256, 256, TG_EPI_BIAS_MUL_GELU_GRAD));
    // the other entry points: the second problem's tiles are appended to the first one's
    show("pair 1024+1280 x256->256", pair(1024, 1280, 256, 256));
    show("pair 1024+1280 x64->256", pair(1024, 1280, 64, 256));
    show("pair 1024+1280 x256->256 w4=0", pair(1024, 1280, 256, 256), 0);
    show("pair silu 1024+1280 x256->256", pair(1024, 1280, 256, 256, TG_EPI_BIAS_SILU));
    show("qkv 1024x256->768 v_col0 512", qkv(1024, 0, 256, 768, 512));
    show("qkv 1024+1280 x256->768 v_col0 512", qkv(1024, 1280, 256, 768, 512));
    show("lora 1024x256->256 R 64", lora(1024, 256, 256, 64));
    show("lora 1024x256->256 R 384", lora(1024, 256, 256, 384));
    show("lora 1024x8192->256 R 64", lora(1024, 8192, 256, 64));
    // ---- refusals: one per message, on each side of its threshold (the other side is a case above) ----
    show("refused: plain M = 0", plain(0, 64, 128));
    show("refused: plain N = 100", plain(4, 64, 100));
    show("refused: plain K = 96", plain(4, 96, 128));
    show("refused: plain epilogue 6", plain(1024, 256, 256, 6));
    show("plain 2147483391x64->65536 (2^31 - 256 tiles)", plain(2147483391, 64, 65536));      // the kernels count tiles in `int`
    show("refused: plain 2147483647x64->65536 (2^31 tiles)", plain(2147483647, 64, 65536));
    const int act_epilogues[] = {TG_EPI_BIAS_KEEP_GELU, TG_EPI_BIAS_MUL_GELU_GRAD};
    for (int epi : act_epilogues) {
        const char* e = epi == TG_EPI_BIAS_KEEP_GELU ? "keep_gelu" : "gelu_grad";
        char name[96];
        snprintf(name, sizeof(name), "refused: plain %s M = 512", e);
        show(name, plain(512, 256, 256, epi));
        snprintf(name, sizeof(name), "refused: plain %s K = 192", e);
        show(name, plain(1024, 192, 256, epi));
        snprintf(name, sizeof(name), "refused: plain %s N = 384", e);
        show(name, plain(1024, 256, 384, epi));
        snprintf(name, sizeof(name), "refused: plain %s w4=0", e);
        show(name, plain(1024, 256, 256, epi), 0);
    }
    show("refused: pair M2 = 1023", pair(1024, 1023, 256, 256));
    show("refused: pair N = 384", pair(1024, 1280, 256, 384));
    show("refused: pair epilogue 3", pair(1024, 1280, 256, 256, TG_EPI_BIAS_GATE_RES));
    show("refused: qkv K = 192", qkv(1024, 0, 192, 768, 512));
    show("refused: qkv M = 1023", qkv(1023, 0, 256, 768, 512));
    show("refused: qkv M2 = 512", qkv(1024, 512, 256, 768, 512));
    show("refused: qkv v_col0 = 0", qkv(1024, 0, 256, 768, 0));
    show("refused: qkv v_col0 = N", qkv(1024, 0, 256, 768, 768));
    show("refused: qkv v_col0 = 384", qkv(1024, 0, 256, 768, 384));
    { GemmShape s = qkv(1024, 0, 256, 768, 512); s.vt_ld1 = 1000; show("refused: qkv vt_ld = 1000", s); }
    { GemmShape s = qkv(1024, 0, 256, 768, 512); s.vt_ld1 = 960; show("refused: qkv vt_ld = 960", s); }
    show("refused: qkv lda = 2^21", with_ld(qkv(1024, 0, 256, 768, 512), LD_LIMIT, 256));
    show("refused: qkv w4=0", qkv(1024, 0, 256, 768, 512), 0);
    show("refused: lora M = 1023", lora(1023, 256, 256, 64));
    show("refused: lora R = 32", lora(1024, 256, 256, 32));
    show("refused: lora R = 96", lora(1024, 256, 256, 96));
    show("refused: lora R = 448", lora(1024, 256, 256, 448));
    { GemmShape s = lora(1024, 256, 256, 64); s.ldt = 56; show("refused: lora ldt = 56", s); }
    { GemmShape s = lora(1024, 256, 256, 64); s.ldb = LD_LIMIT; show("refused: lora ldb = 2^21", s); }
    show("refused: lora w4=0", lora(1024, 256, 256, 64), 0);
    return 0;
}
