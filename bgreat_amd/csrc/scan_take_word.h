// scan_take_word.h -- what a scanner half of bgr_align_greedy_multi_kernel (key table in LDS) needs of an item, in ONE 32-bit word per group:
// the word is put together for all sixteen groups at once in vector code and fetched by one lane read when a half takes the item.
// Plain C++ (no HIP in here): the kernel and the launch planner share the bounds, and a host program can check the fields on their own.
//   bits  0- 8  the resume position: the first position the item may report
//   bits  9-17  the positions left: npos - resume position
//   bits 18-26  the item's dword (resume position / 16) counted from the wave's first read word, were a read's dwords in base order
//   bits 27-31  16 - resume position % 16 (1 .. 16)
// The widths hold because of what the kernel takes: a read of L bases goes there only when (L + 31) / 32 < W and W <= kTakeMaxWords, so
// L <= kTakeMaxReadLen = 480, resume position < npos <= L and positions left <= npos <= L; group q's words start 2 W q dwords behind the
// wave's first, q <= kTakeGroups - 1 = 15, and the resume position's dword is at most 479 / 16 = 29: 15 x 32 + 29 = 509.
#ifndef BGREAT_AMD_SCAN_TAKE_WORD_H
#define BGREAT_AMD_SCAN_TAKE_WORD_H

#include <stdint.h>

#if defined(__HIPCC__)
#define BGR_TAKE_HD __host__ __device__ __forceinline__
#else
#define BGR_TAKE_HD inline
#endif

namespace bgr {

constexpr uint32_t kTakeMaxWords = 16;                           // u64 words per read of a group's LDS row, at most (launch_plan.h: wfast)
constexpr uint32_t kTakeMaxReadLen = 32 * (kTakeMaxWords - 1);   // the longest read the kernel takes
constexpr uint32_t kTakeGroups = 16;                             // groups (reads) per wave
constexpr uint32_t kTakePosBits = 9, kTakeDwordBits = 9, kTakeResBits = 5;
constexpr uint32_t kTakeLeftShift = kTakePosBits, kTakeDwordShift = 2 * kTakePosBits, kTakeResShift = 2 * kTakePosBits + kTakeDwordBits;
constexpr uint32_t kTakePosMask = (1u << kTakePosBits) - 1, kTakeDwordMask = (1u << kTakeDwordBits) - 1;
// the largest dword index a word has to hold
constexpr uint32_t take_max_dword(uint32_t groups, uint32_t words, uint32_t max_len) { return (groups - 1) * 2 * words + ((max_len - 1) >> 4); }

static_assert(kTakeMaxReadLen <= kTakePosMask, "resume position and positions left need more than kTakePosBits");
static_assert(take_max_dword(kTakeGroups, kTakeMaxWords, kTakeMaxReadLen) <= kTakeDwordMask, "the item's dword needs more than kTakeDwordBits");
static_assert(kTakeResShift + kTakeResBits == 32 && 16 < (1u << kTakeResBits), "the four fields fill the word");

// (left is masked: a group without an item to scan has nothing left, or less -- its word is never fetched, and stays well defined)
BGR_TAKE_HD uint32_t take_word_pack(uint32_t resume, uint32_t left, uint32_t dword) {
    return (resume & kTakePosMask) | ((left & kTakePosMask) << kTakeLeftShift) | ((dword & kTakeDwordMask) << kTakeDwordShift) |
           ((16u - (resume & 15u)) << kTakeResShift);
}
BGR_TAKE_HD uint32_t take_word_resume(uint32_t w) { return w & kTakePosMask; }
BGR_TAKE_HD uint32_t take_word_left(uint32_t w) { return (w >> kTakeLeftShift) & kTakePosMask; }
BGR_TAKE_HD uint32_t take_word_dword(uint32_t w) { return (w >> kTakeDwordShift) & kTakeDwordMask; }
BGR_TAKE_HD uint32_t take_word_res(uint32_t w) { return w >> kTakeResShift; }

}  // namespace bgr

#endif
