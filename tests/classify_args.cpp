// The two zngamd_bgzf_classify_records entry points with hostile pattern tables, mismatch bounds, record models, flags, duplicate
// patterns and NULL pointers, and no context: every call must answer ZNGAMD_E_ARG before it touches anything.  A stand-alone program:
// tests/test_cpu_bgzf_classify.py builds the library's host side and this file under AddressSanitizer + UndefinedBehaviorSanitizer and
// runs it as a plain child process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zng_amd.h"

static int failures = 0;

struct Case {
    const char *what;
    const uint8_t *patterns;
    uint32_t patterns_len;
    const zngamd_bgzf_pattern *table;
    uint32_t n;
    int delim;
    uint32_t flags, k, record_lines;
    int32_t match_line, first_byte;
    bool totals;
};

// form 0: host, 1: device
static int call(int form, zngamd_ctx *ctx, const Case &c)
{
    zngamd_bgzf_classify_totals t;
    memset(&t, 0, sizeof t);
    if (form == 0)
        return zngamd_bgzf_classify_records(ctx, nullptr, 0, nullptr, 0, 0, 0, c.patterns, c.patterns_len, c.table, c.n, c.delim, c.flags, c.k, c.record_lines,
                                            c.match_line, c.first_byte, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, c.totals ? &t : nullptr);
    return zngamd_bgzf_classify_records_dev(ctx, nullptr, 0, nullptr, 0, 0, 0, c.patterns, c.patterns_len, c.table, c.n, c.delim, c.flags, c.k, c.record_lines,
                                            c.match_line, c.first_byte, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, c.totals ? &t : nullptr);
}

static void expect_arg(const Case &c, zngamd_ctx *ctx)
{
    for (int form = 0; form < 2; form++) {
        const int r = call(form, ctx, c);
        if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d): %d\n", c.what, form, r); failures++; }
    }
}

int main()
{
    // the blob is exactly as long as patterns_len says: a read behind it is a report
    std::vector<uint8_t> blob(306, 'x');
    memcpy(blob.data(), "needleneedle", 12);
    const uint32_t len = (uint32_t)blob.size();
    std::vector<uint8_t> nl = {'n', 'e', 'e', '\n', 'd', 'l', 'e'};
    const zngamd_bgzf_pattern one = {0, 6};
    std::vector<zngamd_bgzf_pattern> many(1000, zngamd_bgzf_pattern{0, 2});
    const zngamd_bgzf_pattern behind = {len, 1}, over = {len - 2, 3}, wrap = {0xFFFFFFFFu, 2}, wrap2 = {0xFFFFFFF0u, 0x20}, half = {1u << 31, 1u << 31};
    const zngamd_bgzf_pattern empty = {0, 0}, second_empty[2] = {{0, 6}, {3, 0}}, long255 = {12, 255}, long256 = {12, 256}, long300 = {6, 300}, huge = {0, 0xFFFFFFFFu};
    const zngamd_bgzf_pattern with_delim = {0, 7}, delim_alone[2] = {{0, 3}, {3, 1}}, two[2] = {{0, 6}, {12, 2}};
    const zngamd_bgzf_pattern same_row[2] = {{0, 6}, {0, 6}}, same_bytes[2] = {{0, 6}, {6, 6}}, same_far[3] = {{0, 6}, {12, 8}, {6, 6}}, same_x[2] = {{20, 200}, {40, 200}};
    const uint32_t F = ZNGAMD_BGZF_GREP_FINAL, G = ZNGAMD_BGZF_CLASSIFY_GROUP;
    const Case cases[] = {
        {"max_mismatch 17", blob.data(), len, &one, 1, '\n', F, 17, 4, 1, '@', true},
        {"max_mismatch 17 on a pattern of 255", blob.data(), len, &long255, 1, '\n', F, 17, 4, 1, '@', true},
        {"max_mismatch 2^32 - 1", blob.data(), len, &one, 1, '\n', F, 0xFFFFFFFFu, 4, 1, '@', true},
        {"max_mismatch = len", blob.data(), len, &one, 1, '\n', F, 6, 4, 1, '@', true},
        {"max_mismatch > len", blob.data(), len, &one, 1, '\n', F, 7, 4, 1, '@', true},
        {"max_mismatch = the shortest len", blob.data(), len, two, 2, '\n', F, 2, 4, 1, '@', true},
        {"no pattern", blob.data(), len, &one, 0, '\n', F, 1, 4, 1, '@', true},
        {"65 patterns", blob.data(), len, many.data(), 65, '\n', F, 1, 4, 1, '@', true},
        {"1000 patterns", blob.data(), len, many.data(), 1000, '\n', F, 1, 4, 1, '@', true},
        {"length 0", blob.data(), len, &empty, 1, '\n', F, 0, 4, 1, '@', true},
        {"a second pattern of length 0", blob.data(), len, second_empty, 2, '\n', F, 1, 4, 1, '@', true},
        {"length 256", blob.data(), len, &long256, 1, '\n', F, 1, 4, 1, '@', true},
        {"length 300", blob.data(), len, &long300, 1, '\n', F, 1, 4, 1, '@', true},
        {"length 2^32 - 1", blob.data(), len, &huge, 1, '\n', F, 1, 4, 1, '@', true},
        {"a row behind the blob", blob.data(), len, &behind, 1, '\n', F, 0, 4, 1, '@', true},
        {"a row over the blob's end", blob.data(), len, &over, 1, '\n', F, 1, 4, 1, '@', true},
        {"a row whose end wraps", blob.data(), len, &wrap, 1, '\n', F, 1, 4, 1, '@', true},
        {"a row whose end wraps to 16", blob.data(), len, &wrap2, 1, '\n', F, 1, 4, 1, '@', true},
        {"off + len = 2^32", blob.data(), len, &half, 1, '\n', F, 1, 4, 1, '@', true},
        {"a delimiter inside a pattern", nl.data(), 7, &with_delim, 1, '\n', F, 1, 4, 1, '@', true},
        {"a pattern that is the delimiter", nl.data(), 7, delim_alone, 2, '\n', F, 0, 4, 1, '@', true},
        {"delimiter -1", blob.data(), len, &one, 1, -1, F, 1, 4, 1, '@', true},
        {"delimiter 256", blob.data(), len, &one, 1, 256, F, 1, 4, 1, '@', true},
        {"patterns = NULL", nullptr, 6, &one, 1, '\n', F, 1, 4, 1, '@', true},
        {"table = NULL", blob.data(), len, nullptr, 3, '\n', F, 1, 4, 1, '@', true},
        {"totals = NULL", blob.data(), len, &one, 1, '\n', F, 1, 4, 1, '@', false},
        {"record_lines 0", blob.data(), len, &one, 1, '\n', F, 1, 0, -1, '@', true},
        {"record_lines 65", blob.data(), len, &one, 1, '\n', F, 1, 65, 1, '@', true},
        {"record_lines 2^31", blob.data(), len, &one, 1, '\n', F, 1, 1u << 31, 0, '@', true},
        {"match_line -2", blob.data(), len, &one, 1, '\n', F, 1, 4, -2, '@', true},
        {"match_line = record_lines", blob.data(), len, &one, 1, '\n', F, 1, 4, 4, '@', true},
        {"first_byte -2", blob.data(), len, &one, 1, '\n', F, 1, 4, 1, -2, true},
        {"first_byte 256", blob.data(), len, &one, 1, '\n', F, 1, 4, 1, 256, true},
        {"_INVERT", blob.data(), len, &one, 1, '\n', F | ZNGAMD_BGZF_GREP_INVERT, 1, 4, 1, '@', true},
        {"_COUNT_ONLY", blob.data(), len, &one, 1, '\n', G | ZNGAMD_BGZF_GREP_COUNT_ONLY, 1, 4, 1, '@', true},
        {"flag 32", blob.data(), len, &one, 1, '\n', G | 32u, 1, 4, 1, '@', true},
        {"flag 2^31", blob.data(), len, &one, 1, '\n', 1u << 31, 1, 4, 1, '@', true},
        {"the same row twice", blob.data(), len, same_row, 2, '\n', F, 1, 4, 1, '@', true},
        {"two rows of the same bytes", blob.data(), len, same_bytes, 2, '\n', F | G, 1, 4, 1, '@', true},
        {"the same bytes, a pattern between", blob.data(), len, same_far, 3, '\n', F, 0, 4, 1, '@', true},
        {"200 equal bytes at two places", blob.data(), len, same_x, 2, '\n', F, 16, 4, 1, '@', true},
        {"ctx = NULL with everything else in order", blob.data(), len, two, 2, '\n', F | G | ZNGAMD_BGZF_GREP_LINE_START, 1, 4, 1, '@', true},
    };
    uint8_t not_a_context = 0;      // one byte where a context would be: a call that touched it before judging the arguments is a report
    for (const Case &c : cases) {
        expect_arg(c, nullptr);
        if (strncmp(c.what, "ctx = NULL", 10)) expect_arg(c, (zngamd_ctx *)&not_a_context);
    }
    if (sizeof(zngamd_bgzf_class_row) != 4 || sizeof(zngamd_bgzf_classify_totals) != 56 + 16 * ZNGAMD_BGZF_CLASSIFY_MAX_CLASSES) { printf("FAIL layout\n"); failures++; }
    if (failures) return 1;
    printf("bgzf classify arguments clean\n");
    return 0;
}
