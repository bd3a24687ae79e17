// piv_grid.hpp - the host front of every entry point that works on the (win, step) window grid of section 5: the argument
// rules, the grid's size with the size-query convention, the window-size dispatch, and the launch of a kernel that needs
// dynamic LDS.  Users: photon_piv.hip, photon_piv_phase.hip, photon_piv_uncertainty.hip, and section 7's callers
// (photon_piv_deform.hip, photon_optflow.hip).
#pragma once
#include <climits>
#include <cstdio>
#include <type_traits>

#include "photon_internal.hpp"

namespace photon {
namespace piv_grid {

// each rule is nullptr when its arguments are fine
inline const char *win_error(int win) { return win != 16 && win != 32 && win != 64 ? "win must be 16, 32 or 64" : nullptr; }

inline const char *grid_error(int width, int height, int win, int step) {
    if (const char *bad = win_error(win)) return bad;
    if (step < 1) return "step must be >= 1";
    if (width < win || height < win) return "the image is smaller than one window";
    return nullptr;
}

// the same for a caller that brings the grid's size along (section 7)
inline const char *grid_error(int width, int height, int win, int step, int n_rows, int n_cols) {
    if (const char *bad = grid_error(width, height, win, step)) return bad;
    if (n_rows != (height - win) / step + 1 || n_cols != (width - win) / step + 1) return "n_rows x n_cols is not the window grid of section 5";
    return nullptr;
}

// rows x cols of a grid that passed grid_error, also into *n_rows, *n_cols where given (the size query: a caller without
// an output pointer returns 0 after this, nothing launched).  More than INT_MAX windows: one line, nothing written, 1.
inline int grid_size(const char *entry, int width, int height, int win, int step, int &rows, int &cols, int *n_rows, int *n_cols) {
    rows = (height - win) / step + 1, cols = (width - win) / step + 1;
    if ((long long)rows * cols > INT_MAX) {
        fprintf(stderr, "photon: %s: %d x %d windows are too many for one call\n", entry, rows, cols);
        return 1;
    }
    if (n_rows) *n_rows = rows;
    if (n_cols) *n_cols = cols;
    return 0;
}

// f(std::integral_constant<int, win>()) for a win that passed win_error
template <typename F>
int dispatch_win(int win, F f) {
    switch (win) {
    case 16: return f(std::integral_constant<int, 16>());
    case 32: return f(std::integral_constant<int, 32>());
    default: return f(std::integral_constant<int, 64>());
    }
}

inline int lds_limit(int *bytes) {
    int dev = 0;
    PH_CHECK(hipGetDevice(&dev));
    PH_CHECK(hipDeviceGetAttribute(bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    return 0;
}

// the refusal of a window whose kernel needs more LDS than the device has: one line (win and the parameter that sized
// the request), 1
inline int lds_refused(const char *entry, int win, const char *what, int value, int limit) {
    fprintf(stderr, "photon: %s: win %d, %s %d needs more LDS than the device's %d bytes\n", entry, win, what, value, limit);
    return 1;
}

// above 64 KB a kernel gets its dynamic LDS only on request
template <typename Kernel>
int raise_lds(Kernel kernel, size_t bytes) {
    if (bytes > 65536) PH_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

// `kernel` is about to be launched with a fixed `bytes` of dynamic LDS: refuse above the device's limit, raise above 64 KB
template <typename Kernel>
int reserve_lds(Kernel kernel, size_t bytes, const char *entry, int win, const char *what, int value) {
    if (bytes <= 65536) return 0;
    int limit = 0;
    PH_TRY(lds_limit(&limit));
    if (bytes > (size_t)limit) return lds_refused(entry, win, what, value, limit);
    return raise_lds(kernel, bytes);
}

// the sides of an image without a window grid (section 15): pixel coordinates, moved by any halo of the library, stay far
// inside an int.  (Below the launch helpers, whose error lines carry their line numbers.)
inline const char *side_error(int width, int height) {
    if (width < 1 || height < 1) return "width and height must be >= 1";
    if (width > (1 << 22) || height > (1 << 22)) return "the image is larger than 2^22 pixels a side";
    return nullptr;
}

}  // namespace piv_grid
}  // namespace photon
