// Stand-alone host program for tests/test_step_plan_cpu.py: the step planner (csrc/stepplan.h) on the CPU, nothing of HIP.
//   step_plan_main plan key=value ...    describe() of plan_step for the knobs / caps / state given (defaults: the bench width)
//   step_plan_main lds G pk pages        attn_row_lds_bytes
//   step_plan_main sweep                 key soundness over a grid of states: plans compare equal exactly when they describe alike
// Every case ends with "ok <case>"; built with -fsanitize=address,undefined.
#include <cstring>
#include <map>
#include <set>

#include "../../moss-ttsd_amd/csrc/stepplan.h"

struct Setup {
    StepKnobs k;
    StepCaps c;
    StepState s;
    std::vector<char> k_on, v_on;
};

// the bench width on the flagship device: 28 layers, 8 kv heads of 4 q heads, 256 compute units, 160 KiB of LDS per block;
// launch_gemm's kernels at one row tile as the engine reports them there; down_proj and the heads have twins, gate/up none
static Setup bench_setup() {
    Setup u;
    u.c.G = 4; u.c.nkv = 8; u.c.L = 28; u.c.n_cus = 256;
    u.c.small_fits = true; u.c.fold_shape = true; u.c.row_lds_limit = 160 * 1024;
    const bool kinds[WSEAL_KINDS] = {false, true, true, true};
    for (int i = 0; i < WSEAL_KINDS; ++i) { u.c.wseal_kind[i] = kinds[i]; u.s.wseal_on[i] = kinds[i]; }
    u.c.gemm_form[GEMM_O] = GEMM_DEPTH; u.c.gemm_form[GEMM_GU] = GEMM_GATEUP48; u.c.gemm_form[GEMM_DOWN] = GEMM_DEPTH;
    u.s.heads = 1; u.s.B = 32; u.s.R = -1; u.s.pages_bound = 64;
    return u;
}
static void finish(Setup& u) {
    if (u.s.R < 0) u.s.R = (u.s.B + 31) / 32 * 32;
    if (!u.k.gemm_depth) for (int& f : u.c.gemm_form) f = GEMM_SKINNY;       // (mtts_engine_create: the GemmPlans carry the switch)
    if (u.k_on.empty()) u.k_on.assign(u.c.L, 1);
    if (u.v_on.empty()) u.v_on.assign(u.c.L, 1);
    u.k_on.resize(u.c.L, 1); u.v_on.resize(u.c.L, 1);
    if (u.k.kv_pack) { u.s.pack_k_on = u.k_on.data(); u.s.pack_v_on = u.v_on.data(); }
}
static void mask4(bool* out, int m) { for (int i = 0; i < WSEAL_KINDS; ++i) out[i] = (m >> i) & 1; }
static void layers_off(std::vector<char>& v, const char* list, int L) {        // "1,3": those layers' reads go back to bf16
    v.assign(L, 1);
    for (const char* p = list; *p;) {
        const int n = atoi(p);
        if (n >= 0 && n < L) v[n] = 0;
        p = strchr(p, ',');
        if (!p) break;
        ++p;
    }
}
static bool set(Setup& u, const std::string& key, const char* v) {
    const int i = atoi(v);
    std::map<std::string, int*> ints = {
        {"small_rows", &u.k.small_rows}, {"fuse_qkv_max", &u.k.fuse_qkv_max}, {"pack_min_work", &u.k.pack_min_work}, {"attn_row", &u.k.attn_row},
        {"pf_mfma_pages", &u.k.pf_mfma_pages}, {"gemm_depth", &u.k.gemm_depth}, {"fold_norm", &u.k.fold_norm}, {"w_seal_head", &u.k.w_seal_head},
        {"kv_pack", &u.k.kv_pack}, {"G", &u.c.G}, {"nkv", &u.c.nkv}, {"L", &u.c.L}, {"n_cus", &u.c.n_cus}, {"row_lds_limit", &u.c.row_lds_limit},
        {"heads", &u.s.heads}, {"B", &u.s.B}, {"R", &u.s.R}, {"pages", &u.s.pages_bound}, {"topk", &u.s.topk}};
    std::map<std::string, bool*> bools = {{"f32", &u.c.f32}, {"small_fits", &u.c.small_fits}, {"fold_shape", &u.c.fold_shape}, {"lora", &u.s.lora},
                                          {"forced", &u.s.forced}, {"ch0_sampled", &u.s.ch0_sampled}, {"scores", &u.s.scores_on}};
    if (ints.count(key)) *ints[key] = i;
    else if (bools.count(key)) *bools[key] = i != 0;
    else if (key == "wseal_kind") mask4(u.c.wseal_kind, i);
    else if (key == "wseal_on") mask4(u.s.wseal_on, i);
    else if (key == "k_off") layers_off(u.k_on, v, u.c.L);
    else if (key == "v_off") layers_off(u.v_on, v, u.c.L);
    else return false;
    return true;
}

static int sweep() {
    // every combination of the values the other cases probe one at a time, at 4 layers
    const int Bs[] = {1, 4, 5, 31, 32, 33}, pages[] = {15, 16, 80, 81}, rows[] = {0, 1, 2}, seals[] = {0, 14, 15};
    std::vector<StepPlan> plans;                   // one per distinct plan (operator==)
    std::vector<std::string> texts;                // ... and what it describes as
    std::set<std::string> seen;
    long states = 0;
    for (int B : Bs) for (int pg : pages) for (int lora = 0; lora < 2; ++lora) for (int row : rows) for (int depth = 0; depth < 2; ++depth)
    for (int fold = 0; fold < 2; ++fold) for (int seal : seals) for (int koff = 0; koff < 2; ++koff) for (int samp = 0; samp < 2; ++samp) {
        Setup u = bench_setup();
        u.c.L = 4;
        mask4(u.c.wseal_kind, 15);
        u.s.B = B; u.s.pages_bound = pg; u.s.lora = lora; u.k.attn_row = row; u.k.gemm_depth = depth; u.k.fold_norm = fold;
        mask4(u.s.wseal_on, seal);
        if (koff) layers_off(u.k_on, "1", u.c.L);
        u.s.forced = samp; u.s.topk = samp ? 3 : 0;
        finish(u);
        const StepPlan p = plan_step(u.k, u.c, u.s);
        char var[64];
        snprintf(var, sizeof(var), "|%d%d%d%d", p.forced, p.ch0_sampled, p.scores_on, p.topk);
        const std::string text = describe(p) + var;
        ++states;
        size_t hit = plans.size();
        for (size_t i = 0; i < plans.size() && hit == plans.size(); ++i)
            if (plans[i] == p) hit = i;
        if (hit < plans.size()) {
            if (texts[hit] != text) { printf("equal plans describe differently:\n%s\n--\n%s\n", texts[hit].c_str(), text.c_str()); return 1; }
            for (size_t i = hit + 1; i < plans.size(); ++i)
                if (plans[i] == p) { printf("operator== is not transitive\n"); return 1; }
        } else {
            if (seen.count(text)) { printf("different plans describe alike:\n%s\n", text.c_str()); return 1; }
            seen.insert(text);
            plans.push_back(p);
            texts.push_back(text);
        }
    }
    printf("states %ld\ndistinct %d\n", states, (int)plans.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "lds" && argc == 5) printf("%d\n", attn_row_lds_bytes(atoi(argv[2]), atoi(argv[3]) != 0, atoi(argv[4])));
    else if (what == "sweep") { if (sweep()) return 1; }
    else if (what == "plan") {
        Setup u = bench_setup();
        for (int i = 2; i < argc; ++i) {
            const char* eq = strchr(argv[i], '=');
            if (!eq || !set(u, std::string(argv[i], eq - argv[i]), eq + 1)) { printf("bad argument %s\n", argv[i]); return 2; }
        }
        finish(u);
        const StepPlan p = plan_step(u.k, u.c, u.s);
        if (p != plan_step(u.k, u.c, u.s)) { printf("a plan differs from itself\n"); return 1; }
        fputs(describe(p).c_str(), stdout);
    } else return 2;
    printf("ok %s\n", what.c_str());
    return 0;
}
