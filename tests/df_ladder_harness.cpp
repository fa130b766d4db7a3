// tests/df_ladder_harness.cpp -- prints what ilupp_amd/csrc/df_ladder.h states, one line per fact, for tests/test_df_ladder.py to compare
// with tests/capacity_cases.py.  Plain C++ (g++ with AddressSanitizer and UBSan); no GPU, no HIP.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>

#include "df_ladder.h"

using namespace ilupp;

static const long kNnzPerRow[] = {1, 3, 7, 15, 16, 17, 31, 39, 40, 41, 64, 127, 300};
static const long kRows[] = {1, 2, 17, 18, 33, 600, 4096, 100000, 3000000};
static const long kFill[] = {-3, 0, 1, 2, 5, 8, 13, 14, 25, 26, 100};
static const int kStatus[] = {kStOk, kStOwnPart, kStRecordsRead, kStEntries, kStSlots, kStRecordsWritten};

static void table(const char *family, const DfClass *t, int classes)
{
    for (int c = 0; c < classes; ++c) printf("class %s %d %d %d %d %d\n", family, c, t[c].entries, t[c].slots, t[c].records, t[c].waves_per_cu);
}

static void env(const char *family, const char *name, int dflt, int top)
{
    const int values[] = {-1, 0, top - 1, top, top + 1};
    for (int v : values) {
        char text[32];
        snprintf(text, sizeof text, "%d", v);
        setenv(name, text, 1);
        printf("env %s %d %d\n", family, v, start_class_from_env(name, dflt, top));
    }
    unsetenv(name);
    printf("env %s unset %d\n", family, start_class_from_env(name, dflt, top));
}

int main()
{
    static_assert(is_records(kStRecordsRead) && is_records(kStRecordsWritten) && !is_records(kStEntries) && !is_records(kStOk), "records");
    static_assert(is_entries_or_slots(kStOwnPart) && is_entries_or_slots(kStEntries) && is_entries_or_slots(kStSlots) && !is_entries_or_slots(kStRecordsRead) &&
                  !is_entries_or_slots(kStOk) && !is_entries_or_slots(kStStores), "entries or slots");
    printf("status ok %d capacity %d timeout %d pivot_nan %d pivot_dropped %d own_part %d records_read %d entries %d slots %d records_written %d stores %d\n", kStOk,
           kStCapacity, kStTimeout, kStPivotNaN, kStPivotDropped, kStOwnPart, kStRecordsRead, kStEntries, kStSlots, kStRecordsWritten, kStStores);
    printf("attempt outside %d stores %d\n", kOutsideClass, kStoresTooSmall);
    table("iluc", kIlucClass, kCroutClasses);
    table("piluc", kPilucClass, kCroutClasses);
    table("icholt", kIcholtClass, kIcholtClasses);
    for (long n : kRows) {
        for (int c = 0; c < kCroutClasses; ++c) printf("records iluc %ld %d %d\n", n, c, crout_records(kIlucClass, c, n));
        for (int c = 0; c < kCroutClasses; ++c) printf("records piluc %ld %d %d\n", n, c, crout_records(kPilucClass, c, n));
    }
    for (long per : kNnzPerRow)
        for (long n : kRows) {
            const long nnz = per * n + n / 3;
            for (long f : kFill) printf("start iluc %ld %ld %ld %d\n", nnz, n, f, iluc_start_class(nnz, n, f));
            printf("start piluc %ld %ld %d\n", nnz, n, piluc_start_class(nnz, n));
            for (long f : kFill)
                for (int c = 0; c < kIcholtClasses; ++c) printf("records icholt %ld %ld %ld %d %d\n", nnz, n, f, c, icholt_records(nnz, n, f, c));
        }
    for (int c = 0; c < kCroutClasses; ++c)
        for (int s : kStatus) {
            printf("next iluc %d %d %d\n", c, s, iluc_next_class(c, s));
            if (c < kCroutGlobal) printf("next piluc %d %d %d\n", c, s, piluc_next_class(c, s));
        }
    for (int c = 0; c < kIcholtClasses; ++c)
        for (int s : {kStOk, kStCapacity}) printf("next icholt %d %d %d\n", c, s, icholt_next_class(c, s));
    env("iluc", "ILUPP_ILUC_CLASS", 1, kCroutGlobal);
    env("piluc", "ILUPP_PILUC_CLASS", 2, kCroutGlobal);
    env("icholt", "ILUPP_ICHOLT_CLASS", 0, kIcholtClasses);
    printf("df_ladder_harness: ok\n");
    return 0;
}
