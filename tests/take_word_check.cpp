// take_word_check.cpp -- stand-alone host check of bgreat_amd/csrc/scan_take_word.h (tests/test_scan_take_word.py builds and runs it): every
// admissible (resume position, positions left, dword) survives pack and unpack, and the fifth field is 16 - resume position % 16.
#include <stdio.h>

#include <initializer_list>

#include "scan_take_word.h"

int main() {
    using namespace bgr;
    unsigned long long checked = 0;
    const uint32_t max_dword = take_max_dword(kTakeGroups, kTakeMaxWords, kTakeMaxReadLen);
    for (uint32_t npos = 1; npos <= kTakeMaxReadLen; ++npos) {
        for (uint32_t resume = 0; resume < npos; ++resume) {
            // the dwords a group's item can lie in: every group, sixteen words per read and two (the smallest row)
            for (uint32_t words : {2u, kTakeMaxWords}) {
                if (npos > 32 * (words - 1)) continue;
                for (uint32_t q = 0; q < kTakeGroups; ++q) {
                    const uint32_t dword = q * 2 * words + (resume >> 4);
                    if (dword > max_dword) { printf("dword %u above the bound %u\n", dword, max_dword); return 1; }
                    const uint32_t w = take_word_pack(resume, npos - resume, dword);
                    if (take_word_resume(w) != resume || take_word_left(w) != npos - resume || take_word_dword(w) != dword ||
                        take_word_res(w) != 16 - resume % 16) {
                        printf("npos %u resume %u dword %u: word %08x\n", npos, resume, dword, w);
                        return 1;
                    }
                    ++checked;
                }
            }
        }
    }
    // a group without an item to scan: nothing left, or "less" (unsigned wrap) -- the word stays inside its fields
    const uint32_t w = take_word_pack(7, 0u - 3u, 5);
    if (take_word_resume(w) != 7 || take_word_dword(w) != 5 || take_word_res(w) != 9) return 1;
    printf("ok %llu\n", checked);
    return 0;
}
