// The two zngamd_bgzf_qc_records entry points with hostile configurations, delimiters, flags and NULL pointers, and no context: every
// call must answer ZNGAMD_E_ARG before it touches anything.  A stand-alone program: tests/test_cpu_bgzf_qc.py builds the library's host
// side and this file under AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain child process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "zng_amd.h"

static int failures = 0;

struct Args {
    zngamd_bgzf_qc_conf conf;
    bool with_conf = true, with_totals = true, with_tables = true, with_rows = true, with_alloc = false;
    int delim = '\n';
    uint32_t flags = ZNGAMD_BGZF_GREP_FINAL;
};

static void *never(void *, uint64_t) { printf("FAIL the allocator was called\n"); failures++; return nullptr; }

static Args good()
{
    Args a;
    memset(&a.conf, 0, sizeof a.conf);
    a.conf.record_lines = 4; a.conf.seq_line = 1; a.conf.qual_line = 3; a.conf.first_byte = '@'; a.conf.quality_base = 33; a.conf.cycles = 512;
    a.conf.low_quality = 15; a.conf.flags = ZNGAMD_BGZF_QC_ROWS;
    return a;
}

// form 0: host, 1: device
static int call(int form, zngamd_ctx *ctx, const Args &a, const char *what)
{
    zngamd_bgzf_qc_totals t;
    memset(&t, 0x5A, sizeof t);
    // one word of tables and one row with capacities of 0: a call that wrote either before judging the arguments is a report
    std::vector<uint64_t> tables(1, 0x5A5A5A5A5A5A5A5Aull);
    std::vector<zngamd_bgzf_qc_row> rows(1);
    memset(rows.data(), 0x5A, sizeof rows[0]);
    uint64_t *tp = a.with_tables ? tables.data() : nullptr;
    zngamd_bgzf_qc_row *rp = a.with_rows ? rows.data() : nullptr;
    const zngamd_bgzf_qc_conf *cf = a.with_conf ? &a.conf : nullptr;
    int r;
    if (form == 0)
        r = zngamd_bgzf_qc_records(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, 0, nullptr, tp, 0, rp, 0, a.with_alloc ? never : nullptr, nullptr,
                                   a.with_totals ? &t : nullptr);
    else
        r = zngamd_bgzf_qc_records_dev(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, 0, nullptr, 0, nullptr, tp, 0, rp, 0, a.with_totals ? &t : nullptr);
    const uint8_t *b = (const uint8_t *)&t;
    for (size_t i = 0; i < sizeof t; i++)
        if (b[i] != 0x5A) { printf("FAIL %s (form %d): a refused call wrote the totals\n", what, form); failures++; break; }
    const uint8_t *rb = (const uint8_t *)rows.data();
    for (size_t i = 0; i < sizeof rows[0]; i++)
        if (rb[i] != 0x5A) { printf("FAIL %s (form %d): a refused call wrote a row\n", what, form); failures++; break; }
    if (tables[0] != 0x5A5A5A5A5A5A5A5Aull) { printf("FAIL %s (form %d): a refused call wrote the tables\n", what, form); failures++; }
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
    expect_arg("tables = NULL", [](Args &a) { a.with_tables = false; });
    expect_arg("rows = NULL with _QC_ROWS", [](Args &a) { a.with_rows = false; });
    expect_arg("record_lines 0", [](Args &a) { a.conf.record_lines = 0; });
    expect_arg("record_lines 65", [](Args &a) { a.conf.record_lines = 65; });
    expect_arg("record_lines 2^31", [](Args &a) { a.conf.record_lines = 1u << 31; });
    expect_arg("seq_line -1", [](Args &a) { a.conf.seq_line = -1; });
    expect_arg("seq_line 4", [](Args &a) { a.conf.seq_line = 4; });
    expect_arg("qual_line -2", [](Args &a) { a.conf.qual_line = -2; });
    expect_arg("qual_line 4", [](Args &a) { a.conf.qual_line = 4; });
    expect_arg("qual_line == seq_line", [](Args &a) { a.conf.qual_line = 1; });
    expect_arg("first_byte -2", [](Args &a) { a.conf.first_byte = -2; });
    expect_arg("first_byte 256", [](Args &a) { a.conf.first_byte = 256; });
    expect_arg("quality_base 256", [](Args &a) { a.conf.quality_base = 256; });
    expect_arg("quality_base 2^32 - 1", [](Args &a) { a.conf.quality_base = 0xFFFFFFFFu; });
    expect_arg("cycles 0", [](Args &a) { a.conf.cycles = 0; });
    expect_arg("cycles 4097", [](Args &a) { a.conf.cycles = ZNGAMD_BGZF_QC_MAX_CYCLES + 1u; });
    expect_arg("cycles 2^32 - 1", [](Args &a) { a.conf.cycles = 0xFFFFFFFFu; });
    expect_arg("low_quality 94", [](Args &a) { a.conf.low_quality = 94; });
    expect_arg("low_quality 2^31", [](Args &a) { a.conf.low_quality = 1u << 31; });
    expect_arg("conf.flags 2", [](Args &a) { a.conf.flags = 2; });
    expect_arg("conf.flags 2^31 | _QC_ROWS", [](Args &a) { a.conf.flags |= 1u << 31; });
    expect_arg("reserved[0]", [](Args &a) { a.conf.reserved[0] = 1; });
    expect_arg("reserved[7]", [](Args &a) { a.conf.reserved[7] = 1u << 31; });
    expect_arg("delimiter -1", [](Args &a) { a.delim = -1; });
    expect_arg("delimiter 256", [](Args &a) { a.delim = 256; });
    expect_arg("_INVERT", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_INVERT; });
    expect_arg("_LINE_START", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_LINE_START; });
    expect_arg("_COUNT_ONLY", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_COUNT_ONLY; });
    expect_arg("_GROUP", [](Args &a) { a.flags |= ZNGAMD_BGZF_CLASSIFY_GROUP; });
    expect_arg("flag 2^31", [](Args &a) { a.flags = 1u << 31; });
    expect_arg("ctx = NULL with everything else in order", [](Args &) {}, false);
    expect_arg("ctx = NULL, no rows, no qualities", [](Args &a) { a.conf.flags = 0; a.with_rows = false; a.conf.qual_line = -1; a.conf.first_byte = -1; a.flags = 0; }, false);
    {   // the host form takes an allocator in place of the rows; it is not called
        Args a = good();
        a.with_rows = false; a.with_alloc = true;
        const int r = call(0, nullptr, a, "ctx = NULL, rows from the allocator");
        if (r != ZNGAMD_E_ARG) { printf("FAIL ctx = NULL, rows from the allocator: %d\n", r); failures++; }
    }
    if (sizeof(zngamd_bgzf_qc_totals) != 176 || sizeof(zngamd_bgzf_qc_row) != 24 || sizeof(zngamd_bgzf_qc_conf) != 64) { printf("FAIL layout\n"); failures++; }
    if (ZNGAMD_BGZF_QC_TABLE_WORDS(1) != 2u * 100u + 3u + 101u + 94u || ZNGAMD_BGZF_QC_TABLE_WORDS(4096) != 4097ull * 100u + 4098u + 195u) { printf("FAIL words\n"); failures++; }
    if (failures) return 1;
    printf("bgzf qc arguments clean\n");
    return 0;
}
