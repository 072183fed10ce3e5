// launch_taker_check.cpp -- stand-alone host check of bgreat_amd/csrc/launch_taker.h (tests/test_launch_taker.py builds and runs it): the eight
// inputs of the rule that says which of an aligner's two buffer sets takes the next device-resident launch.
#include <stdio.h>

#include "launch_taker.h"

int main() {
    using namespace bgr;
    int checked = 0;
    for (int bits = 0; bits < 8; ++bits) {
        const bool primary_idle = bits & 1, twin_idle = bits & 2, prev_on_twin = bits & 4;
        const Taker t = launch_taker(primary_idle, twin_idle, prev_on_twin);
        const char* why = nullptr;
        if (t != Taker::kPrimary && t != Taker::kTwin) why = "neither of the two";
        else if (primary_idle && t != Taker::kPrimary) why = "the primary is idle and did not take it";
        else if (t == Taker::kTwin && primary_idle) why = "the twin took it although the primary is idle";
        else if (!primary_idle && twin_idle && t != Taker::kTwin) why = "the primary is busy, the twin idle, and the primary took it";
        else if (!primary_idle && !twin_idle && (t == Taker::kTwin) == prev_on_twin) why = "both busy and the taker of the launch before took it again";
        if (why) { printf("primary_idle %d twin_idle %d prev_on_twin %d -> %u: %s\n", primary_idle, twin_idle, prev_on_twin, (unsigned)t, why); return 1; }
        ++checked;
    }
    // a caller that never waits: both stay busy from the second launch on, and the launches take turns
    bool prev_on_twin = false;
    for (int i = 0; i < 16; ++i) {
        const Taker t = launch_taker(i == 0, i <= 1, prev_on_twin);
        if ((t == Taker::kTwin) != (i % 2 == 1)) { printf("launch %d of an un-synced series went to %u\n", i, (unsigned)t); return 1; }
        prev_on_twin = t == Taker::kTwin;
    }
    // a caller that waits between its launches: always the primary, wherever the launch before went
    for (int prev = 0; prev < 2; ++prev)
        if (launch_taker(true, true, prev != 0) != Taker::kPrimary) { printf("a synced launch left the primary\n"); return 1; }
    printf("ok %d\n", checked);
    return 0;
}
