// ilupp_amd/csrc/df_ladder.h -- the capacity ladders of ILUC (iluc_df.hip), one level of partial ILUC (piluc_df.hip) and ICholT
// (icholt_df.hip) as data and pure functions; the routes and their reasons: DESIGN_OTHER_PATHS.md (ICholT, 4c, 4e).  Plain C++ without a
// HIP include: tests/test_df_ladder.py builds it on the CPU and compares it with tests/capacity_cases.py.
#pragma once

#include <stdlib.h>

namespace ilupp {

// the status word an attempt's kernel leaves in ctrl[2] (the first one written wins)
constexpr int kStOk = 0;
constexpr int kStCapacity = 1;          // ICholT: some capacity of the class
constexpr int kStTimeout = 2;           // no progress anywhere within the spin limit
constexpr int kStPivotNaN = 3;          // ICholT: not positive definite
constexpr int kStPivotDropped = 4;      // ICholT: a finite pivot dropped by the threshold or the budget
constexpr int kStOwnPart = 11;          // Crout kernels: A's part of the working vector exceeds the slots
constexpr int kStRecordsRead = 12;      //   more touch records to read than the class holds
constexpr int kStEntries = 13;          //   gathered entries
constexpr int kStSlots = 14;            //   slots of the working vector
constexpr int kStRecordsWritten = 15;   //   a step would get more touch records than the class holds
constexpr int kStStores = 16;           // partial ILUC: the stores of the factors are too small
constexpr bool is_records(int status) { return status == kStRecordsRead || status == kStRecordsWritten; }
constexpr bool is_entries_or_slots(int status) { return status == kStOwnPart || status == kStEntries || status == kStSlots; }

// what an attempt returns besides ILUPP_OK and the library's (negative) errors
constexpr int kOutsideClass = 1;        // the matrix does not fit this class: the ladder goes on
constexpr int kStoresTooSmall = 2;      // partial ILUC: the same class again with larger stores

// A class: the kernel's template arguments and its resident waves per CU.  The last row of a family is its largest class, whose arrays
// are sized at run time: the limits they may grow to (0: the matrix's)
struct DfClass { int entries, slots, records, waves_per_cu; };
constexpr int kCroutClasses = 5, kCroutGlobal = 4, kIcholtClasses = 4, kIcholtGlobal = 3;
constexpr DfClass kIlucClass[kCroutClasses] = {{256, 128, 32, 16}, {768, 256, 64, 8}, {1024, 512, 128, 2}, {960, 256, 512, 2}, {1 << 19, 16384, 4096, 4}};
constexpr DfClass kPilucClass[kCroutClasses] = {{256, 128, 32, 16}, {768, 256, 64, 8}, {1024, 512, 128, 2}, {768, 256, 512, 2}, {1 << 26, 0, 4096, 4}};
constexpr DfClass kIcholtClass[kIcholtClasses] = {{128, 64, 32, 24}, {256, 128, 64, 12}, {1024, 512, 128, 3}, {1 << 18, 2048, 1 << 16, 1}};

// touch records per step of a Crout class; the largest class: as many as steps can reach one, up to its limit
constexpr int crout_records(const DfClass *family, int cls, long n)
{
    if (cls < kCroutGlobal) return family[cls].records;
    int T = 16;
    while (T < family[kCroutGlobal].records && T < n) T *= 2;
    return T;
}

// ILUC starts where a working row of about (entries of A's row + fill) tails of up to fill entries fits
constexpr int iluc_start_class(long nnz, long n, long max_fill_in)
{
    const long fill = max_fill_in < 1 ? 1 : max_fill_in;
    const long est = (nnz / (n > 0 ? n : 1) / 2 + 1 + fill) * fill;
    return est <= 192 ? 0 : (est <= 640 ? 1 : 2);
}
// ... and goes on (kCroutClasses: refused) to class 3 after a records failure, past it (no more entries or slots than class 2) after another
constexpr int iluc_next_class(int cls, int status)
{
    if (is_records(status) && cls < 2) return 3;
    if (is_entries_or_slots(status) && cls == 2) return 4;
    return cls + 1;
}

// partial ILUC starts by the average row (the smallest class has the most waves) and goes on below its largest class
constexpr int piluc_start_class(long nnz, long n)
{
    const long avg = nnz / n + 1;
    return avg <= 16 ? 0 : (avg <= 40 ? 1 : 2);
}
constexpr int piluc_next_class(int cls, int status)
{
    if (is_records(status)) return cls < 2 ? 2 : cls + 1;
    return cls < 2 ? cls + 1 : kCroutGlobal;
}

// ICholT's touch records per row: 16 doubled up to 4 (average column of the triangle + add_fill_in), cut at the class's limit; the largest
// class: as many as the matrix can need, within 8 GB.  kIcholtRefused where classes 0 and 1 hold fewer.  Every failure: the next class
constexpr int kIcholtRefused = -1;
constexpr int icholt_records(long nnz, long n, long add_fill_in, int cls)
{
    const long avg = nnz / n + 1;
    const int limit = cls == kIcholtGlobal ? kIcholtClass[kIcholtGlobal].records : kIcholtClass[2].records;
    int T = 16;
    while (T < 4 * (avg + (add_fill_in > 0 ? add_fill_in : 0)) && T < limit) T *= 2;
    if (cls == kIcholtGlobal) { while (T < limit && T < n && (unsigned long long)n * T * 2 * 32 <= (8ull << 30)) T *= 2; }
    if (cls < 2 && T > kIcholtClass[cls].records) return kIcholtRefused;
    return T;
}
constexpr int icholt_next_class(int cls, int /*status*/) { return cls + 1; }

// ILUPP_ILUC_CLASS, ILUPP_PILUC_CLASS, ILUPP_ICHOLT_CLASS (read per call): unset: dflt; negative: 0; above `top`: top.  ILUC and partial
// ILUC pass their largest class; ICholT passes kIcholtClasses, from where its ladder makes no attempt: refused
inline int start_class_from_env(const char *name, int dflt, int top)
{
    const char *e = getenv(name);
    if (!e) return dflt;
    const int v = atoi(e);
    return v < 0 ? 0 : (v > top ? top : v);
}

}  // namespace ilupp
