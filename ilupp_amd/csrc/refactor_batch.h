// ilupp_amd/csrc/refactor_batch.h -- what the one-workgroup-per-member factorisation launches share (ilu0_batch.hip, ichol0_batch.hip):
// the workgroup's shape, the fetch group, the working row's size in LDS and the address-space typedefs of the arrays behind a descriptor.
#pragma once
#include "common.h"

namespace ilupp {

static constexpr int kRfThreads = 256;         // one wave per SIMD, as k_pivot_apply_batch
static constexpr int kRG = 8;                  // entries of a row fetched together, their loads in flight at once
static constexpr int kRfMaxRow = 31;            // the row cap where LDS allows it
static constexpr size_t kRfRowBytes = (size_t)kRfThreads * (sizeof(double) + 3 * sizeof(int));      // LDS per entry of the longest row

// bytes of LDS in front of the working rows: the flags, to a multiple of 8
__host__ __device__ inline size_t rf_flag_bytes(int n) { return ((size_t)(n > 0 ? n : 1) * sizeof(int) + 7) & ~(size_t)7; }

// The arrays come out of a descriptor in memory, so the compiler cannot tell their address space and would reach them with flat_
// instructions, which count against the LDS counter as well: every wait for a working-row access would wait for the loads in flight.
// Typed as global pointers they are reached with global_ instructions.
#if defined(__HIP_DEVICE_COMPILE__)
#define RF_HBM __attribute__((address_space(1)))
#else
#define RF_HBM
#endif
typedef const RF_HBM int32_t *rf_cint;
typedef const RF_HBM double *rf_cdbl;
typedef RF_HBM double *rf_dbl;
typedef RF_HBM int32_t *rf_int;

}  // namespace ilupp
