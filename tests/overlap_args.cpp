// The two zngamd_bgzf_overlap_records entry points with hostile configurations, delimiters, flags and NULL pointers, and no context:
// every call must answer ZNGAMD_E_ARG before it touches anything.  A stand-alone program: tests/test_cpu_bgzf_overlap.py builds the
// library's host side and this file under AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain child process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>

#include "zng_amd.h"

static int failures = 0;

struct Args {
    zngamd_bgzf_overlap_conf conf;
    bool with_conf = true, with_totals = true;
    int delim = '\n';
    uint32_t flags = ZNGAMD_BGZF_GREP_FINAL;
};

static Args good()
{
    Args a;
    memset(&a.conf, 0, sizeof a.conf);
    a.conf.record_lines = 8; a.conf.seq_line = 1; a.conf.qual_line = 3; a.conf.first_byte = '@'; a.conf.quality_base = 33;
    a.conf.min_overlap = 30; a.conf.max_mismatch = 5; a.conf.max_percent = 20; a.conf.q_high = 30; a.conf.q_low = 14;
    a.conf.flags = ZNGAMD_BGZF_OVERLAP_MERGE | ZNGAMD_BGZF_OVERLAP_CORRECT | ZNGAMD_BGZF_OVERLAP_CUT;
    return a;
}

// form 0: host, 1: device
static int call(int form, zngamd_ctx *ctx, const Args &a, const char *what)
{
    zngamd_bgzf_overlap_totals t;
    memset(&t, 0x5A, sizeof t);
    const zngamd_bgzf_overlap_conf *cf = a.with_conf ? &a.conf : nullptr;
    int r;
    if (form == 0)
        r = zngamd_bgzf_overlap_records(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr,
                                        a.with_totals ? &t : nullptr);
    else
        r = zngamd_bgzf_overlap_records_dev(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0,
                                            a.with_totals ? &t : nullptr);
    const uint8_t *b = (const uint8_t *)&t;
    for (size_t i = 0; i < sizeof t; i++)
        if (b[i] != 0x5A) { printf("FAIL %s (form %d): a refused call wrote the totals\n", what, form); failures++; break; }
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

int main()
{
    expect_arg("conf = NULL", [](Args &a) { a.with_conf = false; });
    expect_arg("totals = NULL", [](Args &a) { a.with_totals = false; });
    expect_arg("record_lines 0", [](Args &a) { a.conf.record_lines = 0; });
    expect_arg("record_lines 1", [](Args &a) { a.conf.record_lines = 1; });
    expect_arg("record_lines 7", [](Args &a) { a.conf.record_lines = 7; });
    expect_arg("record_lines 66", [](Args &a) { a.conf.record_lines = 66; });
    expect_arg("record_lines 2^31", [](Args &a) { a.conf.record_lines = 1u << 31; });
    expect_arg("seq_line -1", [](Args &a) { a.conf.seq_line = -1; });
    expect_arg("seq_line 4 (a line of mate 2)", [](Args &a) { a.conf.seq_line = 4; });
    expect_arg("qual_line -2", [](Args &a) { a.conf.qual_line = -2; });
    expect_arg("qual_line 4", [](Args &a) { a.conf.qual_line = 4; });
    expect_arg("qual_line 7", [](Args &a) { a.conf.qual_line = 7; });
    expect_arg("qual_line == seq_line", [](Args &a) { a.conf.qual_line = 1; });
    expect_arg("first_byte -2", [](Args &a) { a.conf.first_byte = -2; });
    expect_arg("first_byte 256", [](Args &a) { a.conf.first_byte = 256; });
    expect_arg("quality_base 256", [](Args &a) { a.conf.quality_base = 256; });
    expect_arg("min_overlap 0", [](Args &a) { a.conf.min_overlap = 0; });
    expect_arg("min_overlap 1025", [](Args &a) { a.conf.min_overlap = 1025; });
    expect_arg("max_mismatch 1025", [](Args &a) { a.conf.max_mismatch = 1025; });
    expect_arg("max_mismatch 2^32 - 1", [](Args &a) { a.conf.max_mismatch = 0xFFFFFFFFu; });
    expect_arg("max_percent 101", [](Args &a) { a.conf.max_percent = 101; });
    expect_arg("q_high 94", [](Args &a) { a.conf.q_high = 94; });
    expect_arg("q_low 2^31", [](Args &a) { a.conf.q_low = 1u << 31; });
    expect_arg("_CORRECT without a qual_line", [](Args &a) { a.conf.qual_line = -1; });
    expect_arg("conf.flags 16", [](Args &a) { a.conf.flags |= 16u; });
    expect_arg("conf.flags 2^31", [](Args &a) { a.conf.flags = 1u << 31; });
    expect_arg("reserved[0]", [](Args &a) { a.conf.reserved[0] = 1; });
    expect_arg("reserved[4]", [](Args &a) { a.conf.reserved[4] = 1u << 31; });
    expect_arg("delimiter -1", [](Args &a) { a.delim = -1; });
    expect_arg("delimiter 256", [](Args &a) { a.delim = 256; });
    expect_arg("_INVERT", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_INVERT; });
    expect_arg("_LINE_START", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_LINE_START; });
    expect_arg("_COUNT_ONLY", [](Args &a) { a.flags = ZNGAMD_BGZF_CLASSIFY_GROUP | ZNGAMD_BGZF_GREP_COUNT_ONLY; });
    expect_arg("flag 32", [](Args &a) { a.flags |= 32u; });
    expect_arg("flag 2^31", [](Args &a) { a.flags = 1u << 31; });
    expect_arg("ctx = NULL with everything else in order", [](Args &) {}, false);
    expect_arg("ctx = NULL, grouped, both classes", [](Args &a) { a.flags |= ZNGAMD_BGZF_CLASSIFY_GROUP; a.conf.flags |= ZNGAMD_BGZF_OVERLAP_KEEP_UNMERGED; }, false);
    expect_arg("ctx = NULL, FASTA pairs", [](Args &a) { a.conf.record_lines = 4; a.conf.qual_line = -1; a.conf.flags = ZNGAMD_BGZF_OVERLAP_MERGE; a.conf.min_overlap = 1024; a.conf.max_mismatch = 1024; a.conf.max_percent = 100; }, false);
    if (sizeof(zngamd_bgzf_overlap_totals) != 160 || sizeof(zngamd_bgzf_overlap_row) != 16 || sizeof(zngamd_bgzf_overlap_conf) != 64) { printf("FAIL layout\n"); failures++; }
    if (failures) return 1;
    printf("bgzf overlap arguments clean\n");
    return 0;
}
