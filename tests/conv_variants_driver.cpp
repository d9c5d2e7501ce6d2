// Host-only driver of tests/test_conv_variants_cpu.py: walks a fixed grid of conv shapes through the library's dispatch functions
// (no device is touched) and prints what the autotuner would see, or names plan tuples.
//
//   driver grid [-v]     every shape's ordered candidate list with, per candidate: the six plan numbers and partial_bytes, the alternate
//                        weight packing, the walks-reverse flag, the CU share at 256 CUs and the FID_FORCE_NS values 0..40 that select
//                        it; then conv_plan's heuristic picks.  Default: one line per group -- form, map size, batch, residual, plans
//                        shown, hash of the text; -v: the full text (diff two trees by hand).  Opt-in candidates appear under their environment
//                        variables, which the library reads once per process: run one process per environment.
//   driver classify      reads "gen bm bn bk ksplit ns" tuples from stdin, prints each with its variant name ("-" = names nothing)
#include <string>

#include "../scrfd_arcface_facerecognition_amd/csrc/conv.h"

using namespace fid;

namespace {

constexpr int NUM_CUS = 256;
const int SIZES[] = {7, 12, 14, 15, 20, 28, 40, 56, 80, 160};
const int CHANS[] = {32, 64, 96, 128, 224, 256, 512};
const int BATCHES[] = {1, 8, 64};
struct Form { const char *name; int k, stride, pad; };
const Form K3S1{"3x3s1", 3, 1, 1}, K3S2{"3x3s2", 3, 2, 1}, K1S1{"1x1s1", 1, 1, 0}, K1S2{"1x1s2", 1, 2, 0}, K2S2{"2x2s2", 2, 2, 0};
char dummy[64];      // operands are never dereferenced: the dispatch functions only test pointers for null

bool verbose = false;
std::string group_text;
long group_cands = 0;

void emit(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    group_text += buf;
}

void end_group(const char *form, int size, int batch, int res) {
    unsigned long long h = 1469598103934665603ull;      // FNV-1a
    for (unsigned char c : group_text) { h ^= c; h *= 1099511628211ull; }
    printf("%s %d %d %d %ld %016llx\n", form, size, batch, res, group_cands, h);
    if (verbose) fputs(group_text.c_str(), stdout);
    group_text.clear();
    group_cands = 0;
}

ConvArgs conv_args(const Form &f, int size, int batch, int cin, int cout, bool res) {
    ConvArgs a{};
    a.in = a.w = a.out = dummy;
    a.bias = (const float *)dummy;
    a.partial = (float *)dummy;
    a.H = a.W = size;
    a.Ho = a.Wo = (size + 2 * f.pad - f.k) / f.stride + 1;
    a.Cin_p = cin; a.Cout_p = a.w_rows = cout;
    a.kh = a.kw = f.k; a.stride = f.stride; a.pad = f.pad;
    a.M = batch * a.Ho * a.Wo;
    a.act = ACT_RELU;
    if (res) { a.res = dummy; a.res_H = a.Ho; a.res_W = a.Wo; a.res_Cp = cout; }
    a.in_bytes = (unsigned)((size_t)batch * size * size * cin * 2);
    a.w_bytes = (unsigned)((size_t)cout * f.k * f.k * cin * 2);
    return a;
}

void emit_plan(const char *tag, const ConvArgs &a, const ConvPlan &c) {
    emit("%s %d %d %d %d %d %d %zu alt %d rev %d share %.6f force", tag, c.gen, c.bm, c.bn, c.bk, c.ksplit, c.ns, c.partial_bytes, plan_alt_kind(c),
         (int)conv_walks_reverse(c), conv_plan_cu_share(a, c, NUM_CUS));
    for (int ns = 0; ns <= 40; ns++)
        if (conv_force_match(c, -1, ns)) emit(" %d", ns);
    emit("\n");
    group_cands++;
}

// fused: the candidates are also shown as the executor mints them for the fused-shortcut form
void emit_shape(const ConvArgs &a, bool fused = false) {
    emit("shape H %d Cin %d Cout %d rows %d k %d s %d M %d flags %d res %d out2 %d T2 %d Cin2 %d\n", a.H, a.Cin_p, a.Cout_p, a.w_rows, a.kh, a.stride, a.M,
         a.flags, a.res != nullptr, a.out2 != nullptr, a.T2, a.Cin2_p);
    for (const ConvPlan &c : conv_candidates(a, NUM_CUS, true)) {
        emit_plan("c", a, c);
        if (fused) emit_plan("f", a, conv_fused_plan(c));
    }
    emit_plan("h1", a, conv_plan(a, NUM_CUS, true));
    emit_plan("h0", a, conv_plan(a, NUM_CUS, false));
}

void grid() {
    for (const Form *f : {&K3S1, &K3S2, &K1S1, &K1S2, &K2S2})
        for (int size : SIZES)
            for (int batch : BATCHES)
                for (int res = 0; res < 2; res++) {
                    for (int cin : CHANS)
                        for (int cout : CHANS) emit_shape(conv_args(*f, size, batch, cin, cout, res));
                    end_group(f->name, size, batch, res);
                }
    for (int size : SIZES)
        for (int batch : BATCHES) {
            for (const Form *f : {&K3S1, &K1S1})                  // detector head: fp32 output, 32 padded couts
                for (int cin : CHANS) {
                    ConvArgs a = conv_args(*f, size, batch, cin, 32, false);
                    a.flags = CF_OUT_F32; a.act = ACT_NONE;
                    emit_shape(a);
                }
            end_group("head", size, batch, 0);
            for (const Form *f : {&K3S1, &K1S1})                  // residual read at half size (top-down path)
                for (int cin : CHANS)
                    for (int cout : CHANS) {
                        ConvArgs a = conv_args(*f, size, batch, cin, cout, true);
                        a.flags = CF_RES_UP2; a.res_H = a.res_W = (size + 1) / 2;
                        emit_shape(a);
                    }
            end_group("up2", size, batch, 1);
            for (int res = 0; res < 2; res++) {
                for (int cin : CHANS)
                    for (int cout : CHANS) {
                        ConvArgs a = conv_args(K3S1, size, batch, cin, cout, res);
                        a.flags = CF_BORDER;
                        emit_shape(a);
                    }
                end_group("border", size, batch, res);
            }
            for (int cin : CHANS)                                 // shortcut + stride-2 conv in one op: two outputs, 2 * Cout_p weight rows
                for (int cout : CHANS) {
                    ConvArgs a = conv_args(K3S2, size, batch, cin, cout, false);
                    a.out2 = dummy; a.w_rows = 2 * cout;
                    a.w_bytes *= 2;
                    emit_shape(a);
                }
            end_group("out2", size, batch, 0);
            // the block's shortcut conv as T2 extra taps on the block input: behind a stride-1 conv the input is twice the map (1x1 / stride 2, or
            // T2 = 4: average pool + 1x1), behind a stride-2 conv it is that conv's own input size
            struct { const char *name; const Form *f; int t2, in2_size; } const SC[] = {{"sc1", &K3S1, 1, 2 * size}, {"sc4", &K3S1, 4, 2 * size}, {"sc1s2", &K3S2, 1, size}};
            for (const auto &sc : SC) {
                for (int cin2 : CHANS)
                    for (int cout : CHANS) {
                        ConvArgs a = conv_args(*sc.f, size, batch, cout, cout, false);
                        a.in2 = dummy; a.H2 = a.W2 = sc.in2_size; a.Cin2_p = cin2; a.T2 = sc.t2; a.kw2 = sc.t2 == 4 ? 2 : 1; a.s2 = 2;
                        a.in2_bytes = (unsigned)((size_t)batch * a.H2 * a.W2 * cin2 * 2);
                        a.w_bytes = (unsigned)((size_t)cout * (9 * cout + sc.t2 * cin2) * 2);
                        emit_shape(a, true);
                    }
                end_group(sc.name, size, batch, 0);
            }
        }
}

void classify() {
    ConvPlan c{};
    while (scanf("%d %d %d %d %d %d", &c.gen, &c.bm, &c.bn, &c.bk, &c.ksplit, &c.ns) == 6) {
        const ConvVariant *v = conv_variant(c);
        printf("%d %d %d %d %d %d %s\n", c.gen, c.bm, c.bn, c.bk, c.ksplit, c.ns, v ? v->name : "-");
    }
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    verbose = argc > 2 && std::string(argv[2]) == "-v";
    if (mode == "grid") grid();
    else if (mode == "classify") classify();
    else { fprintf(stderr, "usage: %s grid [-v] | classify < tuples\n", argv[0]); return 2; }
    return 0;
}
