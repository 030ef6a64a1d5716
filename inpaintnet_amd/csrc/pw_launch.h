// What the pw_* launchers of the helper-kernel files share: the capped grid of a grid-stride kernel and the launch's status.
#pragma once
#include <hip/hip_runtime.h>

namespace {

inline int grid_for(long n, int block = 256, int cap = 2048) {
    long g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}
inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -2; }

}  // namespace
