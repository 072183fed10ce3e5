// launch_taker.h -- which of an aligner's two sets of launch buffers takes the next bgr_align_device launch: its own (the primary) or its
// twin's (second stream, own results / arena / cursor block / lists / event ring).  Consecutive launches that nobody waited for alternate, so that
// the workgroups of launch i + 1 start on the CU slots that the finished workgroups of launch i free, instead of behind its last straggler.
// Plain C++ (no HIP in here): a pure function of three booleans, so that a host program can enumerate it.
//   primary_idle   the primary's stream has nothing queued or running (hipStreamQuery)
//   twin_idle      the same for the twin's stream (a twin that does not exist yet is idle)
//   prev_on_twin   the twin took the launch before this one
// The rule: the primary whenever it is idle -- a caller that waits or fetches between its launches never leaves the primary's buffers and
// pointers; else the twin if that is idle; else, both busy, whichever did NOT take the launch before (it queues in order behind its own earlier
// launch, whose buffers it reuses: at most two launches are in flight side by side).
#ifndef BGREAT_AMD_LAUNCH_TAKER_H
#define BGREAT_AMD_LAUNCH_TAKER_H

namespace bgr {

enum class Taker : unsigned { kPrimary = 0, kTwin = 1 };

constexpr Taker launch_taker(bool primary_idle, bool twin_idle, bool prev_on_twin) {
    return primary_idle ? Taker::kPrimary : twin_idle ? Taker::kTwin : prev_on_twin ? Taker::kPrimary : Taker::kTwin;
}

static_assert(launch_taker(true, true, true) == Taker::kPrimary && launch_taker(true, false, false) == Taker::kPrimary, "an idle primary takes the launch");
static_assert(launch_taker(false, true, true) == Taker::kTwin, "a busy primary leaves it to an idle twin");
static_assert(launch_taker(false, false, true) == Taker::kPrimary && launch_taker(false, false, false) == Taker::kTwin, "both busy: they take turns");

}  // namespace bgr

#endif
