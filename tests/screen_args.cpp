// The entry points of the contaminant screen -- zngamd_kmer_set_build, _load, _export, _describe, _free and zngamd_bgzf_screen_records[_dev]
// -- with hostile rules, offsets, pairs, configurations, delimiters, flags and NULL pointers, and no context: every call must answer
// ZNGAMD_E_ARG before it touches anything.  A stand-alone program: tests/test_cpu_bgzf_screen.py builds the library's host side and this
// file under AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain child process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "zng_amd.h"

static int failures = 0;
static uint8_t not_a_context = 0;      // one byte where a context would be: a call that touched it before judging the arguments is a report

static bool untouched(const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) if (b[i] != 0x5A) return false;
    return true;
}

// ---- the set
struct Build {
    std::vector<uint8_t> seqs = std::vector<uint8_t>(90, 'A');
    std::vector<uint64_t> offsets = {0, 40, 90};
    uint32_t n_refs = 2, k = 21, flags = ZNGAMD_KMER_CANONICAL;
    bool with_seqs = true, with_offsets = true, with_out = true;
};

static void expect_build(const char *what, const std::function<void(Build &)> &change, bool ctx_too = true)
{
    Build b;
    change(b);
    for (int with_ctx = 0; with_ctx <= (ctx_too ? 1 : 0); with_ctx++) {
        zngamd_kmer_set *out = (zngamd_kmer_set *)(uintptr_t)0x5A5A;
        zngamd_kmer_set_info info;
        memset(&info, 0x5A, sizeof info);
        const int r = zngamd_kmer_set_build(with_ctx ? (zngamd_ctx *)&not_a_context : nullptr, b.with_seqs ? b.seqs.data() : nullptr,
                                            b.with_offsets ? b.offsets.data() : nullptr, b.n_refs, b.k, b.flags, b.with_out ? &out : nullptr, &info);
        if (r != ZNGAMD_E_ARG) { printf("FAIL build, %s (context %d): %d\n", what, with_ctx, r); failures++; }
        if (out != (zngamd_kmer_set *)(uintptr_t)0x5A5A || !untouched(&info, sizeof info)) { printf("FAIL build, %s: a refused call wrote\n", what); failures++; }
    }
}

struct Load {
    std::vector<uint64_t> codes = {1, 2}, masks = {1, 3};
    uint64_t n = 2;
    uint32_t k = 2, flags = ZNGAMD_KMER_CANONICAL, n_refs = 2;
    bool with_arrays = true, with_out = true;
};

static void expect_load(const char *what, const std::function<void(Load &)> &change, bool ctx_too = true)
{
    Load l;
    change(l);
    for (int with_ctx = 0; with_ctx <= (ctx_too ? 1 : 0); with_ctx++) {
        zngamd_kmer_set *out = (zngamd_kmer_set *)(uintptr_t)0x5A5A;
        zngamd_kmer_set_info info;
        memset(&info, 0x5A, sizeof info);
        const int r = zngamd_kmer_set_load(with_ctx ? (zngamd_ctx *)&not_a_context : nullptr, l.k, l.flags, l.n_refs, l.with_arrays ? l.codes.data() : nullptr,
                                           l.with_arrays ? l.masks.data() : nullptr, l.n, l.with_out ? &out : nullptr, &info);
        if (r != ZNGAMD_E_ARG) { printf("FAIL load, %s (context %d): %d\n", what, with_ctx, r); failures++; }
        if (out != (zngamd_kmer_set *)(uintptr_t)0x5A5A || !untouched(&info, sizeof info)) { printf("FAIL load, %s: a refused call wrote\n", what); failures++; }
    }
}

// ---- the screen
struct Args {
    zngamd_bgzf_screen_conf conf;
    bool with_conf = true, with_totals = true, with_rows = true, with_alloc = false;
    int delim = '\n';
    uint32_t flags = ZNGAMD_BGZF_GREP_FINAL;
};

static void *never(void *, uint64_t) { printf("FAIL the allocator was called\n"); failures++; return nullptr; }

static Args good()
{
    Args a;
    memset(&a.conf, 0, sizeof a.conf);
    a.conf.record_lines = 4; a.conf.seq_line = 1; a.conf.first_byte = '@'; a.conf.min_hits = 1;
    return a;
}

// form 0: host, 1: device.  No set can exist without a context, so the set is NULL: one more reason to refuse, and every call must.
static int call(int form, zngamd_ctx *ctx, const Args &a, const char *what)
{
    zngamd_bgzf_screen_totals t;
    memset(&t, 0x5A, sizeof t);
    std::vector<zngamd_bgzf_screen_row> rows(1);         // one row with a capacity of 0: a call that wrote it before judging the arguments is a report
    memset(rows.data(), 0x5A, sizeof rows[0]);
    zngamd_bgzf_screen_row *rp = a.with_rows ? rows.data() : nullptr;
    const zngamd_bgzf_screen_conf *cf = a.with_conf ? &a.conf : nullptr;
    int r;
    if (form == 0)
        r = zngamd_bgzf_screen_records(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, nullptr, 0, nullptr, rp, 0, a.with_alloc ? never : nullptr, nullptr,
                                       a.with_totals ? &t : nullptr);
    else
        r = zngamd_bgzf_screen_records_dev(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, nullptr, 0, nullptr, 0, nullptr, rp, 0,
                                           a.with_totals ? &t : nullptr);
    if (!untouched(&t, sizeof t)) { printf("FAIL %s (form %d): a refused call wrote the totals\n", what, form); failures++; }
    if (!untouched(rows.data(), sizeof rows[0])) { printf("FAIL %s (form %d): a refused call wrote a row\n", what, form); failures++; }
    return r;
}

static void expect_arg(const char *what, const std::function<void(Args &)> &change)
{
    Args a = good();
    change(a);
    for (int form = 0; form < 2; form++) {
        int r = call(form, nullptr, a, what);
        if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d): %d\n", what, form, r); failures++; }
        r = call(form, (zngamd_ctx *)&not_a_context, a, what);
        if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d, with a context): %d\n", what, form, r); failures++; }
    }
}

int main()
{
    expect_build("k = 0", [](Build &b) { b.k = 0; });
    expect_build("k = 32", [](Build &b) { b.k = 32; });
    expect_build("k = 2^31", [](Build &b) { b.k = 1u << 31; });
    expect_build("n_refs = 0", [](Build &b) { b.n_refs = 0; });
    expect_build("n_refs = 65", [](Build &b) { b.n_refs = 65; b.offsets.assign(66, 0); });
    expect_build("n_refs = 2^32 - 1", [](Build &b) { b.n_refs = UINT32_MAX; });
    expect_build("offsets decrease", [](Build &b) { b.offsets = {0, 50, 40}; });
    expect_build("offsets decrease at once", [](Build &b) { b.offsets = {10, 0, 90}; });
    expect_build("offsets = NULL", [](Build &b) { b.with_offsets = false; });
    expect_build("out = NULL", [](Build &b) { b.with_out = false; });
    expect_build("seqs = NULL", [](Build &b) { b.with_seqs = false; });
    expect_build("flags 2", [](Build &b) { b.flags = 2; });
    expect_build("flags 2^31 | _CANONICAL", [](Build &b) { b.flags |= 1u << 31; });
    expect_build("2^28 + 1 positions", [](Build &b) { b.n_refs = 1; b.offsets = {0, ZNGAMD_KMER_MAX_POSITIONS + 21}; });
    expect_build("2^28 + 1 positions in two references", [](Build &b) { b.k = 1; b.offsets = {0, ZNGAMD_KMER_MAX_POSITIONS, ZNGAMD_KMER_MAX_POSITIONS + 1}; });
    expect_build("a reference of 2^63 bytes", [](Build &b) { b.k = 1; b.offsets = {0, 1ull << 63, 1ull << 63}; });
    expect_build("offsets up to 2^64 - 1", [](Build &b) { b.offsets = {0, 5, UINT64_MAX}; });
    expect_build("ctx = NULL with everything else in order", [](Build &) {}, false);
    expect_build("ctx = NULL, no byte at all", [](Build &b) { b.with_seqs = false; b.offsets = {7, 7, 7}; }, false);

    expect_load("k = 0", [](Load &l) { l.k = 0; });
    expect_load("k = 32", [](Load &l) { l.k = 32; });
    expect_load("n_refs = 0", [](Load &l) { l.n_refs = 0; });
    expect_load("n_refs = 65", [](Load &l) { l.n_refs = 65; });
    expect_load("flags 2", [](Load &l) { l.flags = 2; });
    expect_load("out = NULL", [](Load &l) { l.with_out = false; });
    expect_load("no arrays with n = 2", [](Load &l) { l.with_arrays = false; });
    expect_load("a code of 4^k", [](Load &l) { l.codes[1] = 16; });
    expect_load("the all-ones code", [](Load &l) { l.codes[0] = UINT64_MAX; l.k = 31; });
    expect_load("a code of 4^31", [](Load &l) { l.codes[1] = 1ull << 62; l.k = 31; });
    expect_load("a mask of 0", [](Load &l) { l.masks[1] = 0; });
    expect_load("a mask with bit n_refs", [](Load &l) { l.masks[0] = 4; });
    expect_load("a mask with bit 63", [](Load &l) { l.masks[1] = 1ull << 63 | 1; });
    expect_load("n = 2^28 + 1", [](Load &l) { l.n = ZNGAMD_KMER_MAX_POSITIONS + 1; });
    expect_load("n = 2^64 - 1", [](Load &l) { l.n = UINT64_MAX; });
    expect_load("ctx = NULL with everything else in order", [](Load &) {}, false);
    expect_load("ctx = NULL, 64 references, every bit", [](Load &l) { l.n_refs = 64; l.masks[0] = UINT64_MAX; l.k = 31; l.codes[1] = (1ull << 62) - 1; }, false);
    expect_load("ctx = NULL, no pair", [](Load &l) { l.n = 0; l.with_arrays = false; }, false);

    {   // no set: export, describe and free
        uint64_t n = 0x5A5A, code = 0x5A5A, mask = 0x5A5A;
        zngamd_kmer_set_info info;
        memset(&info, 0x5A, sizeof info);
        int r = zngamd_kmer_set_export(nullptr, &code, &mask, 1, &n);
        if (r != ZNGAMD_E_ARG || n != 0x5A5A || code != 0x5A5A || mask != 0x5A5A) { printf("FAIL export of no set: %d\n", r); failures++; }
        r = zngamd_kmer_set_describe(nullptr, &info);
        if (r != ZNGAMD_E_ARG || !untouched(&info, sizeof info)) { printf("FAIL describe of no set: %d\n", r); failures++; }
        zngamd_kmer_set_free(nullptr);
    }

    expect_arg("conf = NULL", [](Args &a) { a.with_conf = false; });
    expect_arg("totals = NULL", [](Args &a) { a.with_totals = false; });
    expect_arg("rows = NULL", [](Args &a) { a.with_rows = false; });
    expect_arg("record_lines 0", [](Args &a) { a.conf.record_lines = 0; });
    expect_arg("record_lines 65", [](Args &a) { a.conf.record_lines = 65; });
    expect_arg("record_lines 2^31", [](Args &a) { a.conf.record_lines = 1u << 31; });
    expect_arg("seq_line -1", [](Args &a) { a.conf.seq_line = -1; });
    expect_arg("seq_line 4", [](Args &a) { a.conf.seq_line = 4; });
    expect_arg("seq_line -2^31", [](Args &a) { a.conf.seq_line = INT32_MIN; });
    expect_arg("first_byte -2", [](Args &a) { a.conf.first_byte = -2; });
    expect_arg("first_byte 256", [](Args &a) { a.conf.first_byte = 256; });
    expect_arg("min_hits 0", [](Args &a) { a.conf.min_hits = 0; });
    expect_arg("conf.flags 1", [](Args &a) { a.conf.flags = 1; });
    expect_arg("conf.flags 2^31", [](Args &a) { a.conf.flags = 1u << 31; });
    expect_arg("reserved[0]", [](Args &a) { a.conf.reserved[0] = 1; });
    expect_arg("reserved[10]", [](Args &a) { a.conf.reserved[10] = 1u << 31; });
    expect_arg("delimiter -1", [](Args &a) { a.delim = -1; });
    expect_arg("delimiter 256", [](Args &a) { a.delim = 256; });
    expect_arg("_INVERT", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_INVERT; });
    expect_arg("_LINE_START", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_LINE_START; });
    expect_arg("_COUNT_ONLY", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_COUNT_ONLY; });
    expect_arg("flag 2^31", [](Args &a) { a.flags = 1u << 31; });
    expect_arg("set = NULL with everything else in order", [](Args &) {});
    expect_arg("set = NULL, the largest min_hits, no options", [](Args &a) { a.conf.min_hits = 0xFFFFFFFFu; a.conf.first_byte = -1; a.flags = 0; });
    {   // the host form takes an allocator in place of the rows; it is not called
        Args a = good();
        a.with_rows = false; a.with_alloc = true;
        const int r = call(0, nullptr, a, "ctx = NULL, rows from the allocator");
        if (r != ZNGAMD_E_ARG) { printf("FAIL ctx = NULL, rows from the allocator: %d\n", r); failures++; }
    }
    if (sizeof(zngamd_bgzf_screen_conf) != 64 || sizeof(zngamd_bgzf_screen_row) != 24 || sizeof(zngamd_bgzf_screen_totals) != 88 || sizeof(zngamd_kmer_set_info) != 48 ||
        sizeof(zngamd_bgzf_screen_totals) != sizeof(zngamd_bgzf_key_totals) + 24) { printf("FAIL layout\n"); failures++; }
    if (failures) return 1;
    printf("bgzf screen arguments clean\n");
    return 0;
}
