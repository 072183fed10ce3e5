// tools/text_epochs_main.cpp -- the book of the text route's epochs, tickets and info blocks (bgreat_amd/csrc/text_epochs.h) played as a program of
// its own (no GPU, no HIP, no Python; tests/test_text_epochs_host.py builds it under AddressSanitizer + UBSan):
//   g++ -std=c++17 -O1 -g -DNDEBUG -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/text_epochs tools/text_epochs_main.cpp
//   /tmp/text_epochs <hook> <call>...    a fresh state whose chain buffer is allocated by the first call, with option test.text_epoch = hook; a call is
//                                        [r]<launches>[x|z]: it takes that many epochs (the first for its parse launch, 3 tickets; the others for format
//                                        launches, 2 tickets each); r: the chain buffer was reallocated in front of it; x: its parse launch failed (no
//                                        tickets, no flip, no further launch); z: the chain state could not be zeroed (the call ends there).
// Prints per call "call zero=<must the chain state be zeroed> block=<b> next=<b> tickets=<parse>,<format>", then "epoch <e>" per launch ("epoch error"
// where next_epoch refuses), then "end block=<b> next=<b>".  -DNDEBUG: what a release build does behind its assert; without it the refusal aborts.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../bgreat_amd/csrc/text_epochs.h"

using bgr::TextEpochs;

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: text_epochs <hook> [r]<launches>[x|z]...\n"); return 2; }
    const uint32_t hook = (uint32_t)strtoul(argv[1], nullptr, 0);
    printf("max %u per_call %u\n", (unsigned)BGR_TEXT_EPOCH_MAX, bgr::kTextEpochsPerCall);
    TextEpochs ep;
    for (int i = 2; i < argc; ++i) {
        const char* s = argv[i];
        const bool realloc_ = i == 2 || s[0] == 'r';
        if (s[0] == 'r') ++s;
        char* end = nullptr;
        const long launches = strtol(s, &end, 10);
        const bool parse_fails = *end == 'x', zero_fails = *end == 'z';
        if (launches < 0 || launches > 8 || (*end && strcmp(end, "x") && strcmp(end, "z"))) { fprintf(stderr, "bad call %s\n", argv[i]); return 2; }
        const bool zero = ep.begin_call(realloc_, hook);
        printf("call zero=%d block=%u next=%u tickets=%u,%u\n", zero ? 1 : 0, ep.block(), ep.next_block(), ep.ticket_base(TextEpochs::kParse), ep.ticket_base(TextEpochs::kFormat));
        if (zero_fails) { ep.zero_failed(); printf("end block=%u next=%u\n", ep.block(), ep.next_block()); continue; }
        for (long j = 0; j < launches; ++j) {
            const uint32_t e = ep.next_epoch();
            if (!e) { puts("epoch error"); continue; }
            printf("epoch %u\n", e);
            if (j == 0 && parse_fails) break;
            if (j == 0) { ep.commit_flip(); ep.took_tickets(TextEpochs::kParse, 3); }
            else ep.took_tickets(TextEpochs::kFormat, 2);
        }
        printf("end block=%u next=%u\n", ep.block(), ep.next_block());
    }
    return 0;
}
