// Microbenchmark: where the waves of a workgroup with the C2 tile solver's footprint land on a CU of gfx950.
// 256 threads, __launch_bounds__(256, 3), ~168 VGPRs, 49 KB of static LDS, grid 4096: three workgroups share a CU, one wave
// of each on every SIMD.  Every wave stores the raw HW_ID word (and XCC_ID, and its start / end time), spins long enough for
// its two neighbours to arrive, and the host decodes:
//   * which SIMD wave index w sits on (4 x 4 table, and the SIMD sequences of waves 0..3 by frequency);
//   * whether a workgroup's four SIMD ids are always a permutation of 0..3;
//   * the threadgroup-slot field of HW_ID (bits 19:16) among workgroups that are resident on one CU at the same time.
// Build: hipcc --offload-arch=gfx950 -O3 -o wave_placement wave_placement.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1;}}while(0)

constexpr int NLIVE = 159;          // live floats per lane across the spin -> the register allocation of the solver
constexpr int LDS_FLOATS = 49 * 256;    // 49 KB
constexpr int GRID = 4096;
constexpr int GETREG_HW_ID = 4 | (31 << 11);      // s_getreg_b32 hwreg(HW_REG_HW_ID, 0, 32)
constexpr int GETREG_XCC_ID = 20 | (31 << 11);    // s_getreg_b32 hwreg(HW_REG_XCC_ID, 0, 32)

struct Rec { unsigned hw_id, xcc_id; unsigned long long t0, t1; };

__global__ void __launch_bounds__(256, 3) probe(const float* __restrict__ in, float* __restrict__ out, Rec* rec, int spin) {
  __shared__ float lds[LDS_FLOATS];
  const int wave = threadIdx.x >> 6;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  const unsigned hw = __builtin_amdgcn_s_getreg(GETREG_HW_ID), xcc = __builtin_amdgcn_s_getreg(GETREG_XCC_ID);
  float w[NLIVE];
  #pragma unroll
  for (int j = 0; j < NLIVE; j++) w[j] = in[(threadIdx.x * NLIVE + j) & 4095];
  for (int j = threadIdx.x; j < LDS_FLOATS; j += 256) lds[j] = w[0];
  __syncthreads();
  #pragma unroll
  for (int j = 0; j < NLIVE; j++) asm volatile("" : "+v"(w[j]));
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  while ((long long)(__builtin_amdgcn_s_memtime() - c0) < spin) __builtin_amdgcn_s_sleep(1);
  #pragma unroll
  for (int j = 0; j < NLIVE; j++) asm volatile("" : "+v"(w[j]));
  float s = lds[(threadIdx.x * 7) % LDS_FLOATS];
  #pragma unroll
  for (int j = 0; j < NLIVE; j++) s += w[j];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
  if ((threadIdx.x & 63) == 0) {
    Rec r; r.hw_id = hw; r.xcc_id = xcc; r.t0 = t0; r.t1 = t1;
    rec[blockIdx.x * 4 + wave] = r;
  }
}

static unsigned bits(unsigned v, int lo, int n) { return (v >> lo) & ((1u << n) - 1); }

int main() {
  float *din, *dout; Rec* drec;
  std::vector<float> hin(4096);
  for (int i = 0; i < 4096; i++) hin[i] = (i % 97) * 0.01f;
  CK(hipMalloc(&din, 4096 * 4)); CK(hipMalloc(&dout, (size_t)GRID * 256 * 4)); CK(hipMalloc(&drec, (size_t)GRID * 4 * sizeof(Rec)));
  CK(hipMemcpy(din, hin.data(), 4096 * 4, hipMemcpyHostToDevice));
  CK(hipMemset(drec, 0, (size_t)GRID * 4 * sizeof(Rec)));
  hipFuncAttributes fa; CK(hipFuncGetAttributes(&fa, (const void*)probe));
  int occ = 0; CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, probe, 256, 0));
  printf("probe kernel: %d VGPRs, %zu B static LDS, %d workgroups per CU by the occupancy query\n", fa.numRegs, fa.sharedSizeBytes, occ);
  probe<<<GRID, 256>>>(din, dout, drec, 2000); CK(hipDeviceSynchronize());      // warm-up
  probe<<<GRID, 256>>>(din, dout, drec, 40000); CK(hipDeviceSynchronize());
  std::vector<Rec> h((size_t)GRID * 4);
  CK(hipMemcpy(h.data(), drec, h.size() * sizeof(Rec), hipMemcpyDeviceToHost));

  // HW_ID (gfx9 layout): wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13, tg 19:16, vm 23:20, queue 26:24, state 29:27, me 31:30
  printf("raw words of workgroups 0..5 (hw_id xcc_id per wave):\n");
  for (int b = 0; b < 6; b++) {
    printf("  wg %d:", b);
    for (int w = 0; w < 4; w++) printf(" %08x %x", h[b * 4 + w].hw_id, h[b * 4 + w].xcc_id);
    printf("\n");
  }
  long table[4][4] = {};
  std::map<std::string, int> seqs;
  int perm = 0, same_cu = 0, same_tg = 0;
  struct Wg { int b; unsigned long long t0, t1; int tg; int simd[4]; int wid[4]; };
  std::map<unsigned, std::vector<Wg>> cus;
  for (int b = 0; b < GRID; b++) {
    Wg g; g.b = b; unsigned seen = 0; std::string s;
    const unsigned hw0 = h[b * 4].hw_id;
    const unsigned key = (bits(h[b * 4].xcc_id, 0, 4) << 12) | (bits(hw0, 13, 3) << 5) | (bits(hw0, 12, 1) << 4) | bits(hw0, 8, 4);
    bool cu_ok = true, tg_ok = true;
    g.t0 = h[b * 4].t0; g.t1 = h[b * 4].t1;
    for (int w = 0; w < 4; w++) {
      const Rec& r = h[b * 4 + w];
      g.simd[w] = bits(r.hw_id, 4, 2); g.wid[w] = bits(r.hw_id, 0, 4);
      table[w][g.simd[w]]++; seen |= 1u << g.simd[w]; s += char('0' + g.simd[w]);
      cu_ok &= bits(r.hw_id, 8, 8) == bits(hw0, 8, 8) && r.xcc_id == h[b * 4].xcc_id;
      tg_ok &= bits(r.hw_id, 16, 4) == bits(hw0, 16, 4);
      g.t0 = std::min(g.t0, r.t0); g.t1 = std::max(g.t1, r.t1);
    }
    g.tg = bits(hw0, 16, 4);
    perm += seen == 0xf; same_cu += cu_ok; same_tg += tg_ok; seqs[s]++;
    cus[key].push_back(g);
  }
  printf("workgroups: %d; SIMD ids of the four waves a permutation of 0..3: %d; all waves on one CU: %d; one tg field per workgroup: %d\n",
         GRID, perm, same_cu, same_tg);
  printf("wave index -> SIMD id (counts):\n");
  for (int w = 0; w < 4; w++) printf("  wave %d: simd0 %ld  simd1 %ld  simd2 %ld  simd3 %ld\n", w, table[w][0], table[w][1], table[w][2], table[w][3]);
  printf("SIMD sequences of waves 0..3 (count):\n");
  for (auto& kv : seqs) printf("  %s %d\n", kv.first.c_str(), kv.second);

  // co-residency: for every workgroup, the workgroups of its CU that were running when it started
  std::map<int, int> tg_hist, nres_hist, start_distinct;
  std::map<std::string, int> rel_hist;
  int tg_clash = 0;
  for (auto& kv : cus) {
    auto& v = kv.second;
    std::sort(v.begin(), v.end(), [](const Wg& a, const Wg& b) { return a.t0 < b.t0; });
    for (size_t i = 0; i < v.size(); i++) {
      tg_hist[v[i].tg]++;
      std::vector<const Wg*> res;
      for (size_t j = 0; j < v.size(); j++) if (v[j].t0 <= v[i].t0 && v[j].t1 > v[i].t0) res.push_back(&v[j]);
      nres_hist[(int)res.size()]++;
      unsigned tgs = 0, starts = 0; bool clash = false;
      for (auto* g : res) { clash |= (tgs >> g->tg) & 1; tgs |= 1u << g->tg; starts |= 1u << g->simd[0]; }
      tg_clash += clash;
      if (res.size() == 3) {
        start_distinct[__builtin_popcount(starts)]++;
        // (SIMD of wave 0 - tg) & 3 of the three resident workgroups, sorted by tg
        std::sort(res.begin(), res.end(), [](const Wg* a, const Wg* b) { return a->tg < b->tg; });
        std::string s;
        for (auto* g : res) { s += "tg" + std::to_string(g->tg) + ":s" + std::to_string(g->simd[0]) + " "; }
        rel_hist[s]++;
      }
    }
  }
  printf("CUs seen: %zu\n", cus.size());
  printf("tg field values (count):"); for (auto& kv : tg_hist) printf("  %d: %d", kv.first, kv.second); printf("\n");
  printf("workgroups resident on the CU when a workgroup starts, itself included (count):"); for (auto& kv : nres_hist) printf("  %d: %d", kv.first, kv.second); printf("\n");
  printf("workgroups that start beside a resident one with the same tg field: %d\n", tg_clash);
  printf("distinct SIMDs of wave 0 among three co-resident workgroups (count):"); for (auto& kv : start_distinct) printf("  %d: %d", kv.first, kv.second); printf("\n");
  printf("three co-resident workgroups, tg field and SIMD of wave 0 (count):\n");
  for (auto& kv : rel_hist) printf("  %s %d\n", kv.first.c_str(), kv.second);
  // two CUs in full, in time order
  int shown = 0;
  for (auto& kv : cus) {
    if (shown++ == 2) break;
    printf("CU key %05x (xcc<<12 | se<<5 | sh<<4 | cu), %zu workgroups, time in 10 ns ticks from the first start:\n", kv.first, kv.second.size());
    const unsigned long long base = kv.second[0].t0;
    for (auto& g : kv.second)
      printf("  wg %4d  start %6llu end %6llu  tg %2d  simd of waves 0..3: %d %d %d %d  wave slots: %d %d %d %d\n", g.b, g.t0 - base, g.t1 - base,
             g.tg, g.simd[0], g.simd[1], g.simd[2], g.simd[3], g.wid[0], g.wid[1], g.wid[2], g.wid[3]);
  }
  return 0;
}
