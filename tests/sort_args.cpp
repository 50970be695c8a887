// The six entry points of the sort -- zngamd_bgzf_sort_key_records[_dev], zngamd_sort_keys[_dev] and zngamd_bgzf_place_records[_dev] -- with
// hostile configurations, delimiters, flags, counts, widths and NULL pointers, and no context: every call must answer ZNGAMD_E_ARG
// before it touches anything.  A stand-alone program: tests/test_cpu_bgzf_sort.py builds the library's host side and this file under
// AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain child process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>

#include "zng_amd.h"

static int failures = 0;

struct Args {
    zngamd_bgzf_sort_conf conf;
    bool with_conf = true, with_totals = true, with_rows = true, with_lengths = true, with_alloc = false;
    int delim = '\n';
    uint32_t flags = ZNGAMD_BGZF_GREP_FINAL;
};

static void *never(void *, uint64_t) { printf("FAIL the allocator was called\n"); failures++; return nullptr; }

static zngamd_bgzf_sort_part bytes_part(int32_t line, int32_t column, uint32_t width)
{
    zngamd_bgzf_sort_part p;
    memset(&p, 0, sizeof p);
    p.line = line; p.column = column; p.width = width; p.kind = ZNGAMD_BGZF_SORT_BYTES; p.sep = '\t';
    return p;
}

static Args good()
{
    Args a;
    memset(&a.conf, 0, sizeof a.conf);
    a.conf.record_lines = 4; a.conf.first_byte = '@'; a.conf.meta_byte = -1; a.conf.n_parts = 3;
    a.conf.part[0] = bytes_part(0, 0, 64); a.conf.part[0].flags = ZNGAMD_BGZF_SORT_IGNORE_CASE | ZNGAMD_BGZF_SORT_TRUNCATE | ZNGAMD_BGZF_SORT_REVERSE;
    a.conf.part[1] = bytes_part(1, -1, 0); a.conf.part[1].kind = ZNGAMD_BGZF_SORT_LENGTH;
    a.conf.part[2] = bytes_part(0, 1, 0); a.conf.part[2].kind = ZNGAMD_BGZF_SORT_NUMBER; a.conf.part[2].flags = ZNGAMD_BGZF_SORT_REVERSE;
    return a;
}

static bool untouched(const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) if (b[i] != 0x5A) return false;
    return true;
}

// form 0: host, 1: device
static int key_call(int form, zngamd_ctx *ctx, const Args &a, const char *what)
{
    zngamd_bgzf_sort_key_totals t;
    memset(&t, 0x5A, sizeof t);
    uint8_t row[256]; uint32_t len[1];                  // one row with a capacity of 0: a call that wrote it before judging the arguments is a report
    memset(row, 0x5A, sizeof row); memset(len, 0x5A, sizeof len);
    uint8_t *rp = a.with_rows ? row : nullptr;
    uint32_t *lp = a.with_lengths ? len : nullptr;
    const zngamd_bgzf_sort_conf *cf = a.with_conf ? &a.conf : nullptr;
    int r;
    if (form == 0)
        r = zngamd_bgzf_sort_key_records(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, 0, nullptr, rp, lp, 0, a.with_alloc ? never : nullptr, nullptr,
                                         a.with_totals ? &t : nullptr);
    else
        r = zngamd_bgzf_sort_key_records_dev(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, 0, nullptr, 0, nullptr, rp, lp, 0, a.with_totals ? &t : nullptr);
    if (!untouched(&t, sizeof t) || !untouched(row, sizeof row) || !untouched(len, sizeof len)) { printf("FAIL %s (form %d): a refused call wrote\n", what, form); failures++; }
    return r;
}

static void expect_key(const char *what, const std::function<void(Args &)> &change, bool ctx_too = true)
{
    Args a = good();
    change(a);
    uint8_t not_a_context = 0;      // one byte where a context would be: a call that touched it before judging the arguments is a report
    for (int form = 0; form < 2; form++) {
        int r = key_call(form, nullptr, a, what);
        if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d): %d\n", what, form, r); failures++; }
        if (!ctx_too) continue;
        r = key_call(form, (zngamd_ctx *)&not_a_context, a, what);
        if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d, with a context): %d\n", what, form, r); failures++; }
    }
}

// the sort: form 0 host, 1 device.  off: the keys' and the work area's addresses are those of aligned buffers plus these.
static void expect_sort(const char *what, bool with_keys, uint64_t n, uint32_t width, bool with_order, bool with_scratch, unsigned key_off, unsigned scratch_off,
                        bool ctx_too, int forms = 3)
{
    uint8_t not_a_context = 0;
    alignas(16) uint8_t area[64], keys[512];
    for (int form = 0; form < 2; form++) {
        if (!(forms >> form & 1)) continue;
        for (int with_ctx = 0; with_ctx <= (ctx_too ? 1 : 0); with_ctx++) {
            zngamd_ctx *ctx = with_ctx ? (zngamd_ctx *)&not_a_context : nullptr;
            memset(area, 0x5A, sizeof area); memset(keys, 0x5A, sizeof keys);
            uint32_t order = 0x5A5A5A5Au, rank = 0x5A5A5A5Au;
            int r;
            if (form == 0) r = zngamd_sort_keys(ctx, with_keys ? keys + key_off : nullptr, n, width, with_order ? &order : nullptr, &rank);
            else r = zngamd_sort_keys_dev(ctx, with_keys ? keys + key_off : nullptr, n, width, with_scratch ? area + scratch_off : nullptr, 0,
                                          with_order ? &order : nullptr, &rank);
            if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d, context %d): %d\n", what, form, with_ctx, r); failures++; }
            if (!untouched(area, sizeof area) || !untouched(keys, sizeof keys) || order != 0x5A5A5A5Au || rank != 0x5A5A5A5Au) {
                printf("FAIL %s (form %d): a refused call wrote\n", what, form); failures++;
            }
        }
    }
}

struct Place { int delim = '\n'; uint32_t flags = ZNGAMD_BGZF_GREP_FINAL, k = 4; int32_t first_byte = '@'; bool dst = true, len = true, out = true, totals = true; uint64_t n = 1, cap = 8; };

static void expect_place(const char *what, const std::function<void(Place &)> &change, bool ctx_too = true)
{
    Place p;
    change(p);
    uint8_t not_a_context = 0;
    for (int form = 0; form < 2; form++) {
        for (int with_ctx = 0; with_ctx <= (ctx_too ? 1 : 0); with_ctx++) {
            zngamd_ctx *ctx = with_ctx ? (zngamd_ctx *)&not_a_context : nullptr;
            zngamd_bgzf_place_totals t;
            memset(&t, 0x5A, sizeof t);
            uint64_t dst = 0; uint32_t len = 4; uint8_t out[8];
            memset(out, 0x5A, sizeof out);
            int r;
            if (form == 0)
                r = zngamd_bgzf_place_records(ctx, nullptr, 0, nullptr, 0, 0, 0, p.delim, p.flags, p.k, p.first_byte, 0, nullptr, p.dst ? &dst : nullptr,
                                              p.len ? &len : nullptr, p.n, p.out ? out : nullptr, p.cap, p.totals ? &t : nullptr);
            else
                r = zngamd_bgzf_place_records_dev(ctx, nullptr, 0, nullptr, 0, 0, 0, p.delim, p.flags, p.k, p.first_byte, 0, nullptr, 0, nullptr,
                                                  p.dst ? &dst : nullptr, p.len ? &len : nullptr, p.n, p.out ? out : nullptr, p.cap, p.totals ? &t : nullptr);
            if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d, context %d): %d\n", what, form, with_ctx, r); failures++; }
            if (!untouched(&t, sizeof t) || !untouched(out, sizeof out)) { printf("FAIL %s (form %d): a refused call wrote\n", what, form); failures++; }
        }
    }
}

int main()
{
    expect_key("conf = NULL", [](Args &a) { a.with_conf = false; });
    expect_key("totals = NULL", [](Args &a) { a.with_totals = false; });
    expect_key("rows = NULL", [](Args &a) { a.with_rows = false; });
    expect_key("lengths = NULL", [](Args &a) { a.with_lengths = false; });
    expect_key("record_lines 0", [](Args &a) { a.conf.record_lines = 0; });
    expect_key("record_lines 65", [](Args &a) { a.conf.record_lines = 65; });
    expect_key("first_byte -2", [](Args &a) { a.conf.first_byte = -2; });
    expect_key("first_byte 256", [](Args &a) { a.conf.first_byte = 256; });
    expect_key("meta_byte -2", [](Args &a) { a.conf.meta_byte = -2; });
    expect_key("meta_byte 256", [](Args &a) { a.conf.meta_byte = 256; });
    expect_key("n_parts 5", [](Args &a) { a.conf.n_parts = 5; });
    expect_key("n_parts 2^31", [](Args &a) { a.conf.n_parts = 1u << 31; });
    expect_key("line -1", [](Args &a) { a.conf.part[0].line = -1; });
    expect_key("line 4", [](Args &a) { a.conf.part[1].line = 4; });
    expect_key("column -2", [](Args &a) { a.conf.part[0].column = -2; });
    expect_key("column -2^31", [](Args &a) { a.conf.part[2].column = INT32_MIN; });
    expect_key("kind 3", [](Args &a) { a.conf.part[0].kind = 3; });
    expect_key("kind 255", [](Args &a) { a.conf.part[2].kind = 255; });
    expect_key("width 0", [](Args &a) { a.conf.part[0].width = 0; });
    expect_key("width 12", [](Args &a) { a.conf.part[0].width = 12; });
    expect_key("width 136", [](Args &a) { a.conf.part[0].width = 136; });
    expect_key("width 2^31", [](Args &a) { a.conf.part[0].width = 1u << 31; });
    expect_key("a width on a number", [](Args &a) { a.conf.part[2].width = 8; });
    expect_key("a first on a length", [](Args &a) { a.conf.part[1].first = 1; });
    expect_key("part flag 8", [](Args &a) { a.conf.part[0].flags = 8; });
    expect_key("part flag 2^15", [](Args &a) { a.conf.part[0].flags |= 1u << 15; });
    expect_key("_IGNORE_CASE on a number", [](Args &a) { a.conf.part[2].flags = ZNGAMD_BGZF_SORT_IGNORE_CASE; });
    expect_key("_TRUNCATE on a length", [](Args &a) { a.conf.part[1].flags = ZNGAMD_BGZF_SORT_TRUNCATE; });
    expect_key("a part behind n_parts", [](Args &a) { a.conf.part[3].width = 8; });
    expect_key("a separator behind n_parts", [](Args &a) { a.conf.part[3].sep = '\t'; });
    expect_key("reserved[0]", [](Args &a) { a.conf.reserved[0] = 1; });
    expect_key("reserved[7]", [](Args &a) { a.conf.reserved[7] = 1u << 31; });
    expect_key("W = 264", [](Args &a) { a.conf.n_parts = 3; a.conf.part[0] = bytes_part(0, -1, 128); a.conf.part[1] = bytes_part(1, -1, 128); a.conf.part[2] = bytes_part(0, 0, 8); });
    expect_key("W = 260", [](Args &a) { a.conf.n_parts = 3; a.conf.part[0] = bytes_part(0, -1, 128); a.conf.part[1] = bytes_part(1, -1, 128); });      // (+ the number: 264 > 256)
    expect_key("delimiter -1", [](Args &a) { a.delim = -1; });
    expect_key("delimiter 256", [](Args &a) { a.delim = 256; });
    expect_key("_INVERT", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_INVERT; });
    expect_key("_LINE_START", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_LINE_START; });
    expect_key("_COUNT_ONLY", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_COUNT_ONLY; });
    expect_key("_GROUP", [](Args &a) { a.flags |= ZNGAMD_BGZF_CLASSIFY_GROUP; });
    expect_key("flag 2^31", [](Args &a) { a.flags = 1u << 31; });
    expect_key("ctx = NULL with everything else in order", [](Args &) {}, false);
    expect_key("ctx = NULL, no part, no rows", [](Args &a) { memset(a.conf.part, 0, sizeof a.conf.part); a.conf.n_parts = 0; a.with_rows = false; a.flags = 0; }, false);
    expect_key("ctx = NULL, W = 256", [](Args &a) { a.conf.n_parts = 2; a.conf.part[0] = bytes_part(0, -1, 128); a.conf.part[1] = bytes_part(1, -1, 128);
                                                      memset(&a.conf.part[2], 0, sizeof a.conf.part[2]); }, false);
    {   // the host form takes an allocator in place of the arrays; it is not called
        Args a = good();
        a.with_rows = a.with_lengths = false; a.with_alloc = true;
        const int r = key_call(0, nullptr, a, "ctx = NULL, rows from the allocator");
        if (r != ZNGAMD_E_ARG) { printf("FAIL ctx = NULL, rows from the allocator: %d\n", r); failures++; }
    }
    expect_sort("keys = NULL with n = 1", false, 1, 8, true, true, 0, 0, true);
    expect_sort("order = NULL with n = 1", true, 1, 8, false, true, 0, 0, true);
    expect_sort("n = 2^30 + 1", true, ZNGAMD_SORT_MAX_KEYS + 1u, 8, true, true, 0, 0, true);
    expect_sort("n = 2^64 - 1", true, UINT64_MAX, 8, true, true, 0, 0, true);
    expect_sort("width 0", true, 1, 0, true, true, 0, 0, true);
    expect_sort("width 4", true, 1, 4, true, true, 0, 0, true);
    expect_sort("width 12", true, 1, 12, true, true, 0, 0, true);
    expect_sort("width 264", true, 1, 264, true, true, 0, 0, true);
    expect_sort("width 2^31", true, 1, 1u << 31, true, true, 0, 0, true);
    expect_sort("scratch = NULL with n = 1", true, 1, 8, true, false, 0, 0, true, 2);
    expect_sort("scratch off by 4", true, 1, 8, true, true, 0, 4, true, 2);
    expect_sort("keys off by 4", true, 1, 8, true, true, 4, 0, true, 2);
    expect_sort("ctx = NULL with everything else in order", true, 1, 8, true, true, 0, 0, false);
    expect_sort("ctx = NULL, no row", false, 0, 256, false, false, 0, 0, false);
    if (zngamd_sort_scratch_bytes(0, 8) != 1024u + 16u || zngamd_sort_scratch_bytes(1, 8) != 8u + 8u + 1024u + 1024u + 16u ||
        zngamd_sort_scratch_bytes(2048, 256) != 8192u + 2048u + 1024u + 1024u + 512u || zngamd_sort_scratch_bytes(2049, 16) != 8200u + 2056u + 2048u + 1024u + 32u ||
        zngamd_sort_scratch_bytes(ZNGAMD_SORT_MAX_KEYS, 256) != (1ull << 32) + (1ull << 30) + (1ull << 29) + 1024u + 512u ||
        zngamd_sort_scratch_bytes(ZNGAMD_SORT_MAX_KEYS + 1u, 8) != 0 || zngamd_sort_scratch_bytes(UINT64_MAX, 8) != 0 || zngamd_sort_scratch_bytes(1, 0) != 0 ||
        zngamd_sort_scratch_bytes(1, 12) != 0 || zngamd_sort_scratch_bytes(1, 264) != 0) { printf("FAIL scratch bytes\n"); failures++; }
    expect_place("totals = NULL", [](Place &p) { p.totals = false; });
    expect_place("dst = NULL with n = 1", [](Place &p) { p.dst = false; });
    expect_place("length = NULL with n = 1", [](Place &p) { p.len = false; });
    expect_place("out = NULL with a capacity", [](Place &p) { p.out = false; });
    expect_place("record_lines 0", [](Place &p) { p.k = 0; });
    expect_place("record_lines 65", [](Place &p) { p.k = 65; });
    expect_place("first_byte -2", [](Place &p) { p.first_byte = -2; });
    expect_place("first_byte 256", [](Place &p) { p.first_byte = 256; });
    expect_place("delimiter -1", [](Place &p) { p.delim = -1; });
    expect_place("delimiter 256", [](Place &p) { p.delim = 256; });
    expect_place("_GROUP", [](Place &p) { p.flags |= ZNGAMD_BGZF_CLASSIFY_GROUP; });
    expect_place("_INVERT", [](Place &p) { p.flags |= ZNGAMD_BGZF_GREP_INVERT; });
    expect_place("flag 2^31", [](Place &p) { p.flags = 1u << 31; });
    expect_place("ctx = NULL with everything else in order", [](Place &) {}, false);
    expect_place("ctx = NULL, no arrays, no output", [](Place &p) { p.dst = p.len = p.out = false; p.n = 0; p.cap = 0; }, false);
    if (sizeof(zngamd_bgzf_sort_part) != 20 || sizeof(zngamd_bgzf_sort_conf) != 128 || sizeof(zngamd_bgzf_sort_key_totals) != 64 ||
        sizeof(zngamd_bgzf_place_totals) != 64) { printf("FAIL layout\n"); failures++; }
    if (failures) return 1;
    printf("bgzf sort arguments clean\n");
    return 0;
}
