// Stand-alone driver of the LoRA entry points' HOST side (argument checks, workspace arithmetic) for the sanitizer build of the library
// (python -m thunder_speech_amd.build --asan): every call below returns before a launch, so it runs without a GPU.
//   clang++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -I include \
//       tools/diag/lora_host_check.cpp thunder_speech_amd/libthunder_speech_hip.asan.so -Wl,-rpath,thunder_speech_amd -o tools/diag/lora_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "thunder_speech_amd/lora_train.h"

static int failures = 0;
#define EXPECT(expr, want)                                                                \
  do {                                                                                    \
    const long long got_ = (long long)(expr);                                             \
    if (got_ != (long long)(want)) {                                                      \
      std::printf("FAIL %s = %lld, expected %lld\n", #expr, got_, (long long)(want));     \
      ++failures;                                                                         \
    }                                                                                     \
  } while (0)

int main() {
  EXPECT(ts_lora_abi_version(), TS_LORA_ABI_VERSION);
  alignas(16) static char buf[64];
  void* p = buf;                 // a non-NULL, 16-byte aligned HOST pointer: never dereferenced by a call that returns before its launch
  void* odd = buf + 4;
  float* f = reinterpret_cast<float*>(buf);
  float* fodd = reinterpret_cast<float*>(buf + 4);
  const int64_t rows = 4;
  // forward
  EXPECT(ts_lora_fwd(nullptr, rows, 128, p, p, 128, 16, 1.f, f, 384, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, rows, 128, nullptr, p, 128, 16, 1.f, f, 384, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, rows, 128, p, nullptr, 128, 16, 1.f, f, 384, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, rows, 128, p, p, 128, 16, 1.f, nullptr, 384, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, rows, 128, p, p, 128, 16, 1.f, f, 384, nullptr, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, 0, 128, p, p, 128, 16, 1.f, f, 384, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, INT64_MIN, 128, p, p, 128, 16, 1.f, f, 384, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, rows, 0, p, p, 128, 16, 1.f, f, 384, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, rows, 128, p, p, -32, 16, 1.f, f, 384, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, rows, 128, p, p, 128, 0, 1.f, f, 384, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, rows, 128, p, p, 128, 16, 1.f, f, 96, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_fwd(p, rows, 128, p, p, 128, 12, 1.f, f, 384, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_fwd(p, rows, 100, p, p, 128, 16, 1.f, f, 384, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_fwd(p, rows, INT32_MAX, p, p, 128, 16, 1.f, f, 384, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_fwd(p, INT64_MAX, 128, p, p, 128, 16, 1.f, f, 384, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_fwd(p, rows, 128, p, p, 128, 16, 1.f, f, 386, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_fwd(odd, rows, 128, p, p, 128, 16, 1.f, f, 384, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_fwd(p, rows, 128, p, p, 128, 16, 1.f, fodd, 384, p, nullptr), TS_EUNSUPPORTED);
  // backward
  EXPECT(ts_lora_bwd(nullptr, 384, p, p, rows, 128, 128, 16, 1.f, p, p, f, f, f, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_bwd(p, 384, nullptr, p, rows, 128, 128, 16, 1.f, p, p, f, f, f, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_bwd(p, 384, p, nullptr, rows, 128, 128, 16, 1.f, p, p, f, f, f, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_bwd(p, 384, p, p, rows, 128, 128, 16, 1.f, nullptr, p, f, f, f, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_bwd(p, 384, p, p, rows, 128, 128, 16, 1.f, p, nullptr, f, f, f, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_bwd(p, 384, p, p, rows, 128, 128, 16, 1.f, p, p, f, nullptr, f, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_bwd(p, 384, p, p, rows, 128, 128, 16, 1.f, p, p, f, f, nullptr, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_bwd(p, 384, p, p, rows, 128, 128, 16, 1.f, p, p, f, f, f, nullptr, nullptr), TS_EINVAL);
  EXPECT(ts_lora_bwd(p, 384, p, p, 0, 128, 128, 16, 1.f, p, p, f, f, f, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_bwd(p, 96, p, p, rows, 128, 128, 16, 1.f, p, p, f, f, f, p, nullptr), TS_EINVAL);
  EXPECT(ts_lora_bwd(p, 384, p, p, rows, 128, 128, 12, 1.f, p, p, f, f, f, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_bwd(p, 384, p, p, rows, 100, 128, 16, 1.f, p, p, f, f, f, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_bwd(p, 384, p, p, rows, 128, 100, 16, 1.f, p, p, f, f, f, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_bwd(p, 388, p, p, rows, 128, 128, 16, 1.f, p, p, f, f, f, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_bwd(p, 384, p, p, rows, 128, 128, 16, 1.f, p, p, fodd, f, f, p, nullptr), TS_EUNSUPPORTED);
  EXPECT(ts_lora_bwd(p, 384, p, p, rows, 128, 128, 16, 1.f, p, p, f, f, f, odd, nullptr), TS_EUNSUPPORTED);
  // workspace arithmetic: g [rows][r] f32 + ranges x r (k + n) f32; 1 range up to 128 rows, at most 32
  EXPECT(ts_lora_bwd_workspace(0, 128, 128, 16), TS_EINVAL);
  EXPECT(ts_lora_bwd_workspace(rows, 0, 128, 16), TS_EINVAL);
  EXPECT(ts_lora_bwd_workspace(rows, 128, -1, 16), TS_EINVAL);
  EXPECT(ts_lora_bwd_workspace(rows, 128, 128, 0), TS_EINVAL);
  EXPECT(ts_lora_bwd_workspace(1, 128, 128, 8), 4LL * (8 + 8 * 256));
  EXPECT(ts_lora_bwd_workspace(300, 320, 320, 64), 4LL * (300 * 64 + 3 * 64 * 640));
  EXPECT(ts_lora_bwd_workspace(3992, 1280, 1280, 16), 4LL * (3992 * 16 + 32 * 16 * 2560));
  EXPECT(ts_lora_bwd_workspace(1LL << 31, 1280, 1280, 64), 4LL * ((1LL << 31) * 64 + 32LL * 64 * 2560));
  if (failures) return 1;
  std::printf("lora host checks ok\n");
  return 0;
}
