// sanitize_haplotag.cpp -- stand-alone driver of the host code of haplotags (bgreat_amd/csrc/haplotag_host.h: the tag table from structs and from
// the bytes of a --blocks file with every check, the tag of a row, the fields of a GAF line), built with -fsanitize=address,undefined by
// tests/test_haplotag_sanitizers.py.  No device, no library: the header alone.  The inputs are heap blocks of exactly their size -- file bytes
// without a terminator, tables of exactly n_unitigs + 1 words -- so a parser that reads beyond its input or a builder that writes beyond the table
// is caught.
//   sanitize_haplotag  ->  prints "haplotag ok"
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "haplotag_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bgr_bubble bubble(int32_t s, int32_t t, int32_t b, int32_t c) { return bgr_bubble{s, t, {b, c}, {1, 1, 1, 1}}; }

// the parser over a heap copy of exactly the text's bytes -> (ok, table as a vector, message)
struct Parsed { bool ok; std::vector<uint32_t> table; std::string msg; };
static Parsed parse(const std::string& text, uint64_t n_unitigs) {
    std::unique_ptr<char[]> bytes(new char[text.size() ? text.size() : 1]);
    memcpy(bytes.get(), text.data(), text.size());
    std::unique_ptr<uint32_t[]> table(new uint32_t[n_unitigs + 1]);
    for (uint64_t i = 0; i <= n_unitigs; ++i) table[i] = 0xDEADBEEFu;   // (the parser zeroes it)
    Parsed p;
    p.ok = bgr::haplotag_table_of_text(bytes.get(), text.size(), n_unitigs, table.get(), &p.msg);
    p.table.assign(table.get(), table.get() + n_unitigs + 1);
    return p;
}
static std::string row(const std::string& block, const std::string& a, const std::string& b) { return block + "\t0\t1\t1\t1\t4\t" + a + "\t" + b + "\t+\t.\n"; }

int main() {
    const std::string H = bgr::blocks_header();
    {   // the file form: what parses
        Parsed p = parse(H + row("1", "2", "3") + row("1", "-6", "5") + row("7", "1", "7"), 7);
        CHECK(p.ok && p.table == (std::vector<uint32_t>{0, 14, 2, 3, 0, 3, 2, 15}));
        std::string t = H + row("1", "2", "3");
        t.pop_back();   // no trailing newline
        p = parse(t, 3);
        CHECK(p.ok && p.table == (std::vector<uint32_t>{0, 0, 2, 3}));
        p = parse(H, 0);
        CHECK(p.ok && p.table == (std::vector<uint32_t>{0}));
        p = parse(H + row("2147483647", "1", "2"), 2);
        CHECK(p.ok && p.table[1] == 0xFFFFFFFEu && p.table[2] == 0xFFFFFFFFu);
        CHECK(bgr::haplotag_count(p.table.data(), 2) == 2);
    }
    {   // ... and what does not, each with its line
        const struct { std::string text; const char* where; } bad[] = {
            {"", "line 1"}, {H.substr(0, H.size() - 1), "line 1"}, {H.substr(0, 5), "line 1"}, {row("1", "2", "3"), "line 1"}, {"#" + H, "line 1"},
            {H + row("0", "2", "3"), "line 2"}, {H + row("2147483648", "2", "3"), "line 2"}, {H + row("-1", "2", "3"), "line 2"},
            {H + row("1", "0", "3"), "line 2"}, {H + row("1", "2", "8"), "line 2"}, {H + row("1", "-8", "2"), "line 2"}, {H + row("1", "2", "-2"), "line 2"},
            {H + row("1", "2", "3") + row("2", "5", "2"), "line 3"}, {H + row("1", "2", "3") + row("1", "3", "5"), "line 3"},
            {H + "\n", "line 2"}, {H + row("1", "2", "3") + "\n" + row("1", "5", "6"), "line 3"},
            {H + row("1", "2", "3") + "1\t0\t1", "line 3"}, {H + row("1", "2", "3") + "1\t0\t1\t1\t1\t4\t5", "line 3"}, {H + "1\t0\t1\t1\t1\t4\t5\t", "line 2"},
            {H + "1\t0\t1\t1\t1\t4\t2\t3\t+", "line 2"}, {H + "1\t0\t1\t1\t1\t4\t2\t3\t+\t.\tx\n", "line 2"}, {H + "\t\t\t\t\t\t\t\t\t\n", "line 2"},
            {H + row("1x", "2", "3"), "line 2"}, {H + row("1", "+2", "3"), "line 2"}, {H + row("1", "2", ""), "line 2"}, {H + row("1", "2", "-"), "line 2"},
            {H + row("1", " 2", "3"), "line 2"}, {H + row("", "2", "3"), "line 2"},
            {H + row(std::string(40, '1'), "2", "3"), "line 2"}, {H + row("1", std::string(30, '9'), "3"), "line 2"}, {H + row("1", "2", "-" + std::string(400, '9')), "line 2"},
            {H + row("1", "9223372036854775808", "3"), "line 2"}, {H + row("18446744073709551617", "2", "3"), "line 2"}, {H + row("4294967297", "2", "3"), "line 2"},
        };
        for (const auto& b : bad) {
            const Parsed p = parse(b.text, 7);
            if (p.ok || p.msg.find(b.where) == std::string::npos) { printf("FAIL refused file: '%s' -> ok %d, '%s'\n", b.text.substr(H.size() < b.text.size() ? H.size() : 0).c_str(), (int)p.ok, p.msg.c_str()); ++failures; }
        }
        // every prefix of a good file is either refused or parses: no read beyond the bytes
        const std::string good = H + row("1", "2", "3") + row("12", "-6", "5");
        for (size_t n = 0; n <= good.size(); ++n) (void)parse(good.substr(0, n), 7);
    }
    {   // the numbers
        int64_t v = 0;
        const std::string s = "-123";
        CHECK(bgr::haplotag_dec(s.data(), s.data() + 4, &v) && v == -123 && bgr::haplotag_dec(s.data() + 1, s.data() + 4, &v) && v == 123);
        CHECK(!bgr::haplotag_dec(s.data(), s.data(), &v) && !bgr::haplotag_dec(s.data(), s.data() + 1, &v));
        const std::string big(25, '9');
        CHECK(bgr::haplotag_dec(big.data(), big.data() + big.size(), &v) && v == (1ll << 62));
        CHECK(bgr::haplotag_abs(INT32_MIN) == 0x80000000ull && bgr::haplotag_abs(-5) == 5);
    }
    {   // the struct form
        const std::vector<bgr_bubble> b = {bubble(1, 4, 2, 3), bubble(4, 7, 5, 6)};
        std::vector<bgr_block_entry> e = {bgr_block_entry{1, 0, 2, 0, 0, 0}, bgr_block_entry{1, 1, 2, 1, BGR_BLOCK_REVERSED | BGR_BLOCK_HAP | BGR_BLOCK_CIRCULAR, 0}};
        std::unique_ptr<uint32_t[]> t(new uint32_t[8]);
        std::string msg;
        CHECK(bgr::haplotag_table_of(b.data(), b.size(), e.data(), e.size(), 7, 1, t.get(), &msg));
        CHECK((std::vector<uint32_t>(t.get(), t.get() + 8) == std::vector<uint32_t>{0, 0, 2, 3, 0, 3, 2, 0}));
        CHECK(bgr::haplotag_table_of(b.data(), b.size(), e.data(), e.size(), 7, 3, t.get(), &msg) && bgr::haplotag_count(t.get(), 7) == 0);
        CHECK(bgr::haplotag_table_of(nullptr, 0, nullptr, 0, 7, 1, t.get(), &msg));
        std::unique_ptr<uint32_t[]> t6(new uint32_t[6]);
        CHECK(!bgr::haplotag_table_of(b.data(), b.size(), e.data(), e.size(), 5, 1, t6.get(), &msg) && msg.find("entry 1") != std::string::npos);   // 6 is beyond n_unitigs: nothing written there
        std::vector<bgr_block_entry> f = e;
        f[1].bubble = 2; CHECK(!bgr::haplotag_table_of(b.data(), b.size(), f.data(), f.size(), 7, 1, t.get(), &msg) && msg.find("no bubble") != std::string::npos);
        f = e; f[0].block = 0; CHECK(!bgr::haplotag_table_of(b.data(), b.size(), f.data(), f.size(), 7, 1, t.get(), &msg));
        f = e; f[0].block = 0x80000000u; CHECK(!bgr::haplotag_table_of(b.data(), b.size(), f.data(), f.size(), 7, 1, t.get(), &msg));
        f = e; f[0].block = 0x7FFFFFFFu; CHECK(bgr::haplotag_table_of(b.data(), b.size(), f.data(), f.size(), 7, 1, t.get(), &msg) && t[3] == 0xFFFFFFFFu);
        const std::vector<bgr_bubble> m = {bubble(1, 4, 2, INT32_MIN), bubble(1, 4, 2, -2), bubble(1, 4, 0, 3), bubble(4, 7, 3, 6)};
        for (uint32_t i = 0; i < 3; ++i) { const bgr_block_entry x = {1, 0, 1, i, 0, 0}; CHECK(!bgr::haplotag_table_of(m.data(), m.size(), &x, 1, 7, 1, t.get(), &msg)); }
        const bgr_block_entry two[2] = {bgr_block_entry{1, 0, 1, 0, 0, 0}, bgr_block_entry{2, 0, 1, 1, 0, 0}};
        CHECK(!bgr::haplotag_table_of(b.data(), 1, two, 2, 7, 1, t.get(), &msg));   // the second entry's bubble is beyond a list of one
        const std::vector<bgr_bubble> c = {bubble(1, 4, 2, 3), bubble(4, 7, 3, 6)};
        CHECK(!bgr::haplotag_table_of(c.data(), c.size(), two, 2, 7, 1, t.get(), &msg) && msg.find("two different tags") != std::string::npos);
    }
    {   // the tag of a row and the fields of the line
        const std::vector<uint32_t> table = {0, 0, 2, 3, 0, 4, 5, 0, 6};   // block 1: 2 A, 3 B; block 2: 5 A, 6 B; block 3: 8 A (the last entry)
        auto tag = [&](std::vector<int32_t> ids) {
            std::unique_ptr<int32_t[]> h(new int32_t[ids.size() ? ids.size() : 1]);
            for (size_t i = 0; i < ids.size(); ++i) h[i] = ids[i];
            return bgr::haplotag_row(table.data(), 8, h.get(), ids.size());
        };
        bgr_read_tag t = tag({1, 2, 4, 5, 7});
        CHECK(t.block == 1 && t.a == 1 && t.b == 0 && t.others == 1);
        t = tag({-7, -6, -4, -3, -1, 3});
        CHECK(t.block == 1 && t.a == 0 && t.b == 2 && t.others == 1);
        t = tag({8, -8, 0, 9, -9, INT32_MIN, 2147483647});
        CHECK(t.block == 3 && t.a == 2 && t.b == 0 && t.others == 0);
        t = tag({});
        CHECK(t.block == 0 && t.a == 0 && t.b == 0 && t.others == 0);
        t = tag({1, 4, 7});
        CHECK(t.block == 0);
        std::string s = "x\tNM:i:0";
        bgr::haplotag_suffix(t, &s);
        CHECK(s == "x\tNM:i:0");
        bgr::haplotag_suffix(bgr_read_tag{3, 2, 0, 1}, &s);
        CHECK(s == "x\tNM:i:0\tPS:i:3\tHP:i:1\tha:i:2\thb:i:0\tho:i:1");
        s.clear();
        bgr::haplotag_suffix(bgr_read_tag{2147483647u, 4294967295u, 4294967295u, 4294967295u}, &s);
        CHECK(s == "\tPS:i:2147483647\tHP:i:0\tha:i:4294967295\thb:i:4294967295\tho:i:4294967295");
        CHECK(bgr::haplotag_hp(bgr_read_tag{1, 0, 1, 0}) == 2);
    }

    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("haplotag ok\n");
    return 0;
}
