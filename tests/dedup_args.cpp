// The four entry points of duplicate removal -- zngamd_bgzf_key_records[_dev] and zngamd_dedup_keys[_dev] -- with hostile configurations,
// delimiters, flags, counts and NULL pointers, and no context: every call must answer ZNGAMD_E_ARG before it touches anything.  A
// stand-alone program: tests/test_cpu_bgzf_dedup.py builds the library's host side and this file under AddressSanitizer +
// UndefinedBehaviorSanitizer and runs it as a plain child process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "zng_amd.h"

static int failures = 0;

struct Args {
    zngamd_bgzf_key_conf conf;
    bool with_conf = true, with_totals = true, with_rows = true, with_alloc = false;
    int delim = '\n';
    uint32_t flags = ZNGAMD_BGZF_GREP_FINAL;
};

static void *never(void *, uint64_t) { printf("FAIL the allocator was called\n"); failures++; return nullptr; }

static Args good()
{
    Args a;
    memset(&a.conf, 0, sizeof a.conf);
    a.conf.record_lines = 4; a.conf.seq_line = 1; a.conf.first_byte = '@'; a.conf.first = 3; a.conf.length = 50;
    a.conf.flags = ZNGAMD_BGZF_KEY_IGNORE_CASE | ZNGAMD_BGZF_KEY_CANONICAL;
    return a;
}

static bool untouched(const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) if (b[i] != 0x5A) return false;
    return true;
}

// form 0: host, 1: device
static int call(int form, zngamd_ctx *ctx, const Args &a, const char *what)
{
    zngamd_bgzf_key_totals t;
    memset(&t, 0x5A, sizeof t);
    std::vector<zngamd_bgzf_key_row> rows(1);            // one row with a capacity of 0: a call that wrote it before judging the arguments is a report
    memset(rows.data(), 0x5A, sizeof rows[0]);
    zngamd_bgzf_key_row *rp = a.with_rows ? rows.data() : nullptr;
    const zngamd_bgzf_key_conf *cf = a.with_conf ? &a.conf : nullptr;
    int r;
    if (form == 0)
        r = zngamd_bgzf_key_records(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, 0, nullptr, rp, 0, a.with_alloc ? never : nullptr, nullptr,
                                    a.with_totals ? &t : nullptr);
    else
        r = zngamd_bgzf_key_records_dev(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, 0, nullptr, 0, nullptr, rp, 0, a.with_totals ? &t : nullptr);
    if (!untouched(&t, sizeof t)) { printf("FAIL %s (form %d): a refused call wrote the totals\n", what, form); failures++; }
    if (!untouched(rows.data(), sizeof rows[0])) { printf("FAIL %s (form %d): a refused call wrote a row\n", what, form); failures++; }
    return r;
}

static void expect_arg(const char *what, const std::function<void(Args &)> &change, bool ctx_too = true)
{
    Args a = good();
    change(a);
    uint8_t not_a_context = 0;      // one byte where a context would be: a call that touched it before judging the arguments is a report
    for (int form = 0; form < 2; form++) {
        int r = call(form, nullptr, a, what);
        if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d): %d\n", what, form, r); failures++; }
        if (!ctx_too) continue;
        r = call(form, (zngamd_ctx *)&not_a_context, a, what);
        if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d, with a context): %d\n", what, form, r); failures++; }
    }
}

// the two resolve calls: form 0 host, 1 device.  scratch_off: the work area's address is that of an aligned buffer plus this.
static void expect_dedup(const char *what, bool with_keys, uint64_t n, bool with_totals, bool with_scratch, unsigned scratch_off, bool ctx_too)
{
    uint8_t not_a_context = 0;
    alignas(16) uint8_t area[64];
    for (int form = 0; form < 2; form++) {
        for (int with_ctx = 0; with_ctx <= (ctx_too ? 1 : 0); with_ctx++) {
            zngamd_ctx *ctx = with_ctx ? (zngamd_ctx *)&not_a_context : nullptr;
            zngamd_dedup_totals t;
            memset(&t, 0x5A, sizeof t);
            memset(area, 0x5A, sizeof area);
            zngamd_bgzf_key_row key;
            memset(&key, 0x5A, sizeof key);
            uint64_t first = 0x5A5A5A5A5A5A5A5Aull;
            uint32_t count = 0x5A5A5A5Au;
            int r;
            if (form == 0) r = zngamd_dedup_keys(ctx, with_keys ? &key : nullptr, n, &first, &count, with_totals ? &t : nullptr);
            else r = zngamd_dedup_keys_dev(ctx, with_keys ? &key : nullptr, n, with_scratch ? area + scratch_off : nullptr, 0, &first, &count, with_totals ? &t : nullptr);
            if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d, context %d): %d\n", what, form, with_ctx, r); failures++; }
            if (!untouched(&t, sizeof t) || !untouched(area, sizeof area) || first != 0x5A5A5A5A5A5A5A5Aull || count != 0x5A5A5A5Au) {
                printf("FAIL %s (form %d): a refused call wrote\n", what, form); failures++;
            }
        }
    }
}

int main()
{
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
    expect_arg("conf.flags 4", [](Args &a) { a.conf.flags = 4; });
    expect_arg("conf.flags 2^31 | _KEY_CANONICAL", [](Args &a) { a.conf.flags |= 1u << 31; });
    expect_arg("reserved[0]", [](Args &a) { a.conf.reserved[0] = 1; });
    expect_arg("reserved[9]", [](Args &a) { a.conf.reserved[9] = 1u << 31; });
    expect_arg("delimiter -1", [](Args &a) { a.delim = -1; });
    expect_arg("delimiter 256", [](Args &a) { a.delim = 256; });
    expect_arg("_INVERT", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_INVERT; });
    expect_arg("_LINE_START", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_LINE_START; });
    expect_arg("_COUNT_ONLY", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_COUNT_ONLY; });
    expect_arg("_GROUP", [](Args &a) { a.flags |= ZNGAMD_BGZF_CLASSIFY_GROUP; });
    expect_arg("flag 2^31", [](Args &a) { a.flags = 1u << 31; });
    expect_arg("ctx = NULL with everything else in order", [](Args &) {}, false);
    expect_arg("ctx = NULL, the largest part, no options", [](Args &a) { a.conf.first = a.conf.length = 0xFFFFFFFFu; a.conf.flags = 0; a.conf.first_byte = -1; a.flags = 0; }, false);
    {   // the host form takes an allocator in place of the rows; it is not called
        Args a = good();
        a.with_rows = false; a.with_alloc = true;
        const int r = call(0, nullptr, a, "ctx = NULL, rows from the allocator");
        if (r != ZNGAMD_E_ARG) { printf("FAIL ctx = NULL, rows from the allocator: %d\n", r); failures++; }
    }
    expect_dedup("totals = NULL", true, 1, false, true, 0, true);
    expect_dedup("keys = NULL with n = 1", false, 1, true, true, 0, true);
    expect_dedup("n = 2^30 + 1", true, ZNGAMD_DEDUP_MAX_KEYS + 1u, true, true, 0, true);
    expect_dedup("n = 2^64 - 1", true, UINT64_MAX, true, true, 0, true);
    expect_dedup("ctx = NULL with everything else in order", true, 1, true, true, 0, false);
    expect_dedup("ctx = NULL, no key", false, 0, true, false, 0, false);
    {   // the device form alone: no work area for a key; a work area that is not 8-byte aligned
        zngamd_dedup_totals t;
        zngamd_bgzf_key_row key = {1, 2};
        alignas(16) uint8_t area[32];
        uint8_t not_a_context = 0;
        memset(&t, 0x5A, sizeof t);
        int r = zngamd_dedup_keys_dev((zngamd_ctx *)&not_a_context, &key, 1, nullptr, 0, nullptr, nullptr, &t);
        if (r != ZNGAMD_E_ARG || !untouched(&t, sizeof t)) { printf("FAIL scratch = NULL with n = 1: %d\n", r); failures++; }
        r = zngamd_dedup_keys_dev((zngamd_ctx *)&not_a_context, &key, 1, area + 4, sizeof area - 4, nullptr, nullptr, &t);
        if (r != ZNGAMD_E_ARG || !untouched(&t, sizeof t)) { printf("FAIL scratch off by 4: %d\n", r); failures++; }
    }
    if (zngamd_dedup_scratch_bytes(0) != 64u * 12u + 64u || zngamd_dedup_scratch_bytes(32) != 64u * 12u + 64u || zngamd_dedup_scratch_bytes(33) != 128u * 12u + 64u ||
        zngamd_dedup_scratch_bytes(4096) != 8192u * 12u + 64u || zngamd_dedup_scratch_bytes(4097) != 16384u * 12u + 64u ||
        zngamd_dedup_scratch_bytes(ZNGAMD_DEDUP_MAX_KEYS) != (1ull << 31) * 12u + 64u || zngamd_dedup_scratch_bytes(ZNGAMD_DEDUP_MAX_KEYS + 1u) != 0 ||
        zngamd_dedup_scratch_bytes(UINT64_MAX) != 0) { printf("FAIL scratch bytes\n"); failures++; }
    if (sizeof(zngamd_bgzf_key_totals) != 64 || sizeof(zngamd_bgzf_key_row) != 16 || sizeof(zngamd_bgzf_key_conf) != 64 || sizeof(zngamd_dedup_totals) != 48) {
        printf("FAIL layout\n"); failures++;
    }
    if (failures) return 1;
    printf("bgzf dedup arguments clean\n");
    return 0;
}
