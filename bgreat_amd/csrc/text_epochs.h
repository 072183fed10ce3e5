// text_epochs.h -- the host's book of the text route's two one-launch kernels (parse and format, text_kernels.hip): the epoch their chains are
// tagged with, the tickets earlier launches took, and which of the two info blocks a piece uses.  No HIP, no device, no object of the library:
// numbers in, numbers out (tools/text_epochs_main.cpp plays it; tests/test_text_epochs_host.py).  This is the only code that changes them.
//
// Epochs.  A chain word carries the epoch of the launch that wrote it in 22 bits (chain_word, text_kernels.hip); a word of another epoch counts as
// "nothing yet", so the chains are never cleared between launches: every launch gets the next epoch, 1 .. BGR_TEXT_EPOCH_MAX, and the chain state is
// zeroed when a call could run out of them.  An epoch outside the 22 bits would never be matched and every tile behind the first would wait for ever,
// so: a call reserves all the epochs it can use BEFORE its first launch (kTextEpochsPerCall: parse, format, and format once more when the exhaustive
// last pass handed reads back and the launch had to be settled), next_epoch refuses to leave the reservation, and the launchers refuse an epoch out
// of range (launch_text_parse, launch_text_format).
//
// Info blocks.  A piece's parse launch adds to the block of this piece and clears the block of the NEXT one, so that no fill stands in front of
// either (both start zero: bgr_aligner_create).  The flip is committed only once that launch is enqueued: a call that fails before it, the launch
// itself included, leaves the flip where it was, and the block it would have used is still the zero block the launch before it cleared.  (A launch
// that was enqueued and fails later on the device leaves a stream on which every later call fails too: there is no path on which a call that returns
// BGR_OK reads a block that was not cleared.)
#ifndef BGREAT_AMD_TEXT_EPOCHS_H
#define BGREAT_AMD_TEXT_EPOCHS_H

#include <assert.h>
#include <stdint.h>

#define BGR_TEXT_EPOCH_MAX 0x3FFFFFu /* epochs of the chains: 22 bits, 0 = never written */

namespace bgr {

constexpr uint32_t kTextFormatRuns = 2;                        // bgr_align_fasta_text runs its format step at most twice: again behind a settled launch
constexpr uint32_t kTextEpochsPerCall = kTextFormatRuns + 1;   // ... and the parse launch in front of them

class TextEpochs {
public:
    enum Launch { kParse = 0, kFormat = 1 };
    // The start of a call, behind the (re)allocation of the chain state and in front of its first launch.  state_reallocated: the buffer is a new
    // one -- the epoch starts from hook_value (option test.text_epoch: 0 but in tests) and no ticket has been taken.  Then, if fewer than
    // kTextEpochsPerCall epochs are left, the epoch and the ticket bases start from 0 again.  -> whether the caller must zero the chain state
    // before the first launch (when it cannot, it says so: zero_failed)
    bool begin_call(bool state_reallocated, uint32_t hook_value) {
        used_ = 0;
        if (state_reallocated) { epoch_ = hook_value; ticket_[0] = ticket_[1] = 0; }
        const bool wrap = epoch_ > BGR_TEXT_EPOCH_MAX || BGR_TEXT_EPOCH_MAX - epoch_ < kTextEpochsPerCall;
        if (wrap) { epoch_ = 0; ticket_[0] = ticket_[1] = 0; }
        return state_reallocated || wrap;
    }
    void zero_failed() { epoch_ = BGR_TEXT_EPOCH_MAX; }   // the chain state could not be zeroed: the next call asks for it again
    // -> the epoch of the call's next launch, 1 .. BGR_TEXT_EPOCH_MAX; 0 when the call has used its reservation (BGR_E_INTERNAL for the caller: no launch)
    uint32_t next_epoch() {
        const bool ok = used_ < kTextEpochsPerCall && epoch_ < BGR_TEXT_EPOCH_MAX;
        assert(ok && "text route: more launches in a call than epochs reserved for it");
        if (!ok) return 0;
        ++used_;
        return ++epoch_;
    }
    uint32_t ticket_base(Launch which) const { return ticket_[which]; }
    void took_tickets(Launch which, uint32_t n) { ticket_[which] += n; }   // behind a launch that was enqueued: as many as its workgroups take
    uint32_t block() const { return flip_ ^ 1u; }    // the info block of this piece
    uint32_t next_block() const { return flip_; }    // ... of the piece after it: what this piece's parse launch clears
    void commit_flip() { flip_ ^= 1u; }              // behind the parse launch, enqueued without error: the next piece is "this piece" from here on

private:
    uint32_t epoch_ = 0, used_ = 0, ticket_[2] = {0, 0}, flip_ = 0;
};

}  // namespace bgr

#endif
