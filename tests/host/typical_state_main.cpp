// Stand-alone host program for tests/test_sampler_typical_cpu.py: the pending typical_p of csrc/runstate.h on the CPU, nothing
// of HIP.  `typical_state_main` ends with "ok", exit status 0; a check that does not hold prints itself and exits 1.
// Built with -fsanitize=address,undefined.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../moss-ttsd_amd/csrc/runstate.h"

static char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);         \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

int main() {
    PendingRun p;
    CHECK(p.take(2).typical.empty() && p.take_typical().empty());
    // set, taken once by a static run: the next take has none; 0 and 1 are stored as 0 ("absent")
    const float t[8] = {0.9f, 0.f, 1.f, 0.5f, 0.25f, 0.f, 0.f, 0.999f};
    CHECK(p.set_typical(t) == 0);
    RunOptions o = p.take(2);
    CHECK(o.typical.size() == 8 && o.typical[0] == 0.9f && o.typical[1] == 0.f && o.typical[2] == 0.f && o.typical[3] == 0.5f && o.typical[7] == 0.999f);
    CHECK(o.floors.empty() && !o.bans.any());
    CHECK(p.take(2).typical.empty());
    // ... by a scheduler run
    CHECK(p.set_typical(t) == 0);
    CHECK(p.take_typical().size() == 8 && p.take_typical().empty() && p.take(1).typical.empty());
    // a take whose check fails has consumed it all the same
    CHECK(p.set_typical(t) == 0);
    p.set_takes(4);
    o = p.take(3);
    CHECK(o.check(8, false) != 0 && o.typical.size() == 8);
    CHECK(p.take(3).typical.empty());
    // NULL: none, and it clears what was pending
    CHECK(p.set_typical(t) == 0 && p.set_typical(nullptr) == 0 && p.take(1).typical.empty());
    // a refused table names the channel and the field and leaves nothing pending, not even the table set before it
    const float bad[5] = {1.5f, -0.25f, NAN, INFINITY, -0.f - 1e-30f};
    for (int i = 0; i < 5; ++i) {
        float b[8];
        memcpy(b, t, sizeof(b));
        b[5] = bad[i];
        CHECK(p.set_typical(t) == 0);
        g_err[0] = 0;
        CHECK(p.set_typical(b) == RUN_EINVAL);
        CHECK(strstr(g_err, "channel 5") && strstr(g_err, "typical_p"));
        CHECK(p.take(1).typical.empty());
    }
    // the floors' and the bans' one-shots do not touch it, nor it them
    MttsSamplerFloors f[8] = {};
    f[2].min_p = 0.1f;
    CHECK(p.set_floors(f) == 0 && p.set_typical(t) == 0);
    CHECK(p.take_floors().size() == 8 && p.take_typical().size() == 8);
    puts("ok");
    return 0;
}
