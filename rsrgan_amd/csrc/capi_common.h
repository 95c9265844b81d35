// capi_common.h -- what the files behind include/rsrgan.h share: capi.cpp (the handle ABI), capi_front.cpp (the handle-free front end and
// histograms) and capi_ops.cpp (the unit-test operator entries, rsrgan_op_*).  set_error / get_error / HIPC are model.h's.
#pragma once
#include <cstring>
#include <exception>
#include <new>
#include <vector>

#include "model.h"
#include "segan.h"

using namespace rsr;

// Nothing may throw across the C ABI (include/rsrgan.h): every entry point that can allocate host memory runs its body
// through guard(), which turns std::bad_alloc / any other exception into RSRGAN_ERR_INVALID with a message.
template <class F>
static int guard(const char* what, F&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory", what);
  } catch (const std::exception& e) {
    set_error("%s: %s", what, e.what());
  } catch (...) {
    set_error("%s: unknown C++ exception", what);
  }
  return RSRGAN_ERR_INVALID;
}

// ---- argument checks of the handle-free entries: every refusal returns before the first HIP call, so it is testable without a device
#define OP_REFUSE(cond, ...) do { if (cond) { set_error(__VA_ARGS__); return RSRGAN_ERR_INVALID; } } while (0)
// the tail of an entry that launched: OP_LAUNCH_OK where more follows, OP_LAUNCHED where the entry ends
#define OP_LAUNCH_OK(who) do { if (hipGetLastError() != hipSuccess) { set_error(who " launch failed"); return RSRGAN_ERR_HIP; } } while (0)
#define OP_LAUNCHED(who) do { OP_LAUNCH_OK(who); return RSRGAN_OK; } while (0)

// the checks of the table-form entries (op, ptrs, dims, fl).  They name their entry through WHO, a string literal the entry defines
// for the length of its body, and the argument through `name`.
#define OP_DIM(name, v, lo) OP_REFUSE((v) < (lo) || (v) > ((int64_t)1 << 30), WHO ": %s = %lld outside %d .. 2^30", name, (long long)(v), (int)(lo))
#define OP_PTR(name, ptr, align) do { OP_REFUSE(!(ptr), WHO ": null pointer (%s)", name); \
                                      OP_REFUSE((size_t)(ptr) & ((align) - 1), WHO ": %s not %d-byte aligned", name, (int)(align)); } while (0)
#define OP_OPT(name, ptr, align) OP_REFUSE((size_t)(ptr) & ((align) - 1), WHO ": %s not %d-byte aligned", name, (int)(align))
#define OP_LD(name, ld, need) OP_REFUSE((ld) < (need) || (ld) > ((int64_t)1 << 30), WHO ": leading dimension %s = %lld below its row of %lld (or above 2^30)", name, (long long)(ld), (long long)(need))
#define OP_FLAG(name, v) OP_REFUSE((v) < 0 || (v) > 1, WHO ": %s = %lld is neither 0 nor 1", name, (long long)(v))
#define OP_MUL4(name, v) OP_REFUSE((v) & 3, WHO ": %s = %lld is not a multiple of 4", name, (long long)(v))
#define OP_TABLES(nf) OP_REFUSE(!ptrs || !dims || ((nf) && !fl), WHO ": null table (ptrs, dims, or fl for an op that takes floats)")
