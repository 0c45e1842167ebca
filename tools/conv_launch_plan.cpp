// Host launch plans of csrc/kernels/conv_igemm.hip, recorded on the CPU (no GPU is opened):
// the file is compiled host-only with hipLaunchKernelGGL redefined to print the kernel
// instantiation, grid, block and dynamic-LDS bytes instead of launching.  One launch per
// stdin line (tools/conv_launch_plan.py writes them); see that script for the use.
//
//   igemm <variant> <E stats bn_x bn_y bn_mean bn_relu bn_ss bn_mb add_mb: 0 / 1>
//         <Nb H W C P Q R S sa ra oa ob N OH OW os oph opw ldd>
//   bnpro <variant> <stats y: 0 / 1> <Nb H W C P Q R S stride pad N>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <typeinfo>

template <auto KERNEL>
struct Named {};  // its mangled name holds the kernel's, template arguments included

template <auto KERNEL>
static void record(dim3 grid, dim3 block, int lds) {
  printf(" %s grid=%u block=%u lds=%d", typeid(Named<KERNEL>).name(), grid.x, block.x, lds);
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) record<kernel>(grid, block, lds)
#define hipFuncSetAttribute(...) hipSuccess

#include KFA_CONV_IGEMM_HIP

int main() {
  static bf16_t buf[8];
  char line[512], kind[16];
  while (fgets(line, sizeof line, stdin)) {
    int v[32], n = 0, used = 0, step = 0;
    if (sscanf(line, "%15s%n", kind, &used) != 1) continue;
    while (n < 32 && sscanf(line + used, "%d%n", &v[n], &step) == 1) used += step, n++;
    line[strcspn(line, "\n")] = 0;
    printf("%s ->", line);
    auto p = [&](int i) { return v[i] ? buf : nullptr; };
    int rc = -100;
    if (!strcmp(kind, "igemm") && n == 29) {
      const int* g = v + 10;
      rc = kfa_conv_igemm(buf, buf, buf, p(1), g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11],
                          g[12], g[13], g[14], g[15], g[16], g[17], g[18], v[0], (float*)p(2), p(3), p(4),
                          (const float*)p(5), v[6], (const float*)p(7), (const uint8_t*)p(8), (const uint8_t*)p(9),
                          nullptr);
    } else if (!strcmp(kind, "bnpro") && n == 14) {
      const int* g = v + 3;
      rc = kfa_conv_igemm_bnpro(buf, buf, buf, (const float*)buf, p(2), g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7],
                                g[8], g[9], g[10], v[0], (float*)p(1), nullptr);
    }
    printf(" rc=%d\n", rc);
  }
  return 0;
}
