// mpcqp_part.hip -- the one-wave kernels (solver, B = 1 server, fused fleet loop) of horizons
// [MPCQP_PART_LO, MPCQP_PART_HI] (the library is built from several such objects in parallel).
#include "mpcqp_solve.h"

#if !defined(MPCQP_PART_LO) || !defined(MPCQP_PART_HI)
#error "define MPCQP_PART_LO and MPCQP_PART_HI"
#endif

#ifdef MPCQP_STAMPS
// diagnostic builds: this object's own g_stamps (every translation unit has its copy) joins the
// registry mpcqp_debug_stamps sums over
extern "C" void mpcqp_register_stamps(hipError_t (*f)(unsigned long long*, int));
namespace {
hipError_t part_stamps(unsigned long long* out32, int reset) {
  hipError_t e = hipSuccess;
  if (out32) {
    unsigned long long v[32];
    e = hipMemcpyFromSymbol(v, HIP_SYMBOL(g_stamps), sizeof(v));
    for (int i = 0; i < 32 && e == hipSuccess; ++i) out32[i] += v[i];
  }
  if (e == hipSuccess && reset) {
    unsigned long long z[32] = {0};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z));
  }
  return e;
}
const int kRegistered = (mpcqp_register_stamps(part_stamps), 0);
}  // namespace
#endif


namespace {
// the kernels of this object's horizons, instantiated by being registered (mpcqp_solve.h)
const int kHorizonsRegistered = mpcqp::register_horizons<MPCQP_PART_LO, MPCQP_PART_HI>();
}  // namespace
