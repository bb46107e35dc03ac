// Device interop (gft_from_device / gft_to_device): a bit copy between a caller's strided device tensor and a handle's
// compact buffer.  The host side plans the copy (drops unit axes, merges axes that are contiguous on both sides, picks a
// form) and launches one kernel of gft_interop.hip on the library's stream; the C ABI around it (validation, the stream
// joins) is in gft_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gft_kernels.hpp"  // MAXD
#include "gft_series_args.hpp"  // IMAXD (HIP-free: the series argument layer sizes its arrays by it)

namespace gft {

static_assert(IMAXD == MAXD + 1, "the shape's axes after collapsing, plus the lo / hi plane axis of an interval tensor");

enum InteropForm { IO_DENSE = 0, IO_ROWS = 1, IO_TILE = 2 };

// A copy of `nd` axes: element (i_0, ..., i_{nd-1}) moves from src[sum i_a * ss[a]] to dst[sum i_a * ds[a]].  Element
// strides, non-negative; one of the two sides is C-contiguous (the handle's compact buffer).
struct CopyGeom {
    int nd = 0;
    size_t ext[32 + 1];
    size_t ss[32 + 1], ds[32 + 1];
};

// Plans and launches the copy on `st` (through the launch thread); returns the form it took.  Throws std::runtime_error
// if the merged rank exceeds IMAXD.
int interop_copy(hipStream_t st, const double* src, double* dst, const CopyGeom& g);

}  // namespace gft
