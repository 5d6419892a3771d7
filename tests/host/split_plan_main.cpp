// The `split` key of the step plan (csrc/stepplan.h), on the CPU: a stand-alone program that includes that header and nothing
// of HIP.  One case per run: `split_plan_main <case>` ends with "ok <case>", exit status 0; a failed check prints its line.
//   key        split travels from StepState into the plan of a decode step, takes part in its equality and in its text, and
//              changes nothing else of the plan; a prefill pass has none
#include <cstdio>
#include <cstring>
#include <string>

#include "../../moss-ttsd_amd/csrc/stepplan.h"

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } \
    } while (0)

static int key_case() {
    StepKnobs k;
    StepCaps c;
    c.G = 4; c.nkv = 8; c.L = 4; c.n_cus = 256; c.small_fits = true;
    StepState s;
    s.heads = 1; s.B = 3; s.R = 32; s.pages_bound = 2; s.ch0_sampled = true;
    const StepPlan plain = plan_step(k, c, s);
    s.split = true;
    const StepPlan split = plan_step(k, c, s);
    CHECK(!plain.split && split.split);
    CHECK(plain != split && !(plain == split));
    StepPlan same = split;
    same.split = false;
    CHECK(same == plain);                                   // nothing else of the plan moved
    CHECK(describe(plain).find("split") == std::string::npos);
    CHECK(describe(split).find("sample: ch0_sampled topk=0 split\n") != std::string::npos);
    // the fp32 engine's plan carries it too
    c.f32 = true;
    CHECK(plan_step(k, c, s).split);
    s.split = false;
    CHECK(!plan_step(k, c, s).split);
    // a prefill pass has no sampler: the key stays off whatever the state says
    c.f32 = false; s.split = true; s.heads = 2;
    CHECK(!plan_step(k, c, s).split);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: split_plan_main key\n"); return 2; }
    int rc = 2;
    if (!strcmp(argv[1], "key")) rc = key_case();
    if (rc == 0) printf("ok %s\n", argv[1]);
    return rc;
}
