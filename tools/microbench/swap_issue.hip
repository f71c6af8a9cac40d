// Microbenchmark: what the half-wave / row swaps cost the vector port of a gfx950 SIMD, next to the instructions the
// transpose-reduce of the tile solver is made of, and the three candidate reduce sequences as one wave's stream beside
// two waves of packed FMAs (the mix of a SIMD at the C2 shape).
//   part 1: independent streams of v_permlane32_swap, v_permlane16_swap, v_add_f32_dpp, v_cndmask_b32, v_pk_add_f32 and
//           v_pk_fma_f32 at 1, 2 and 3 waves per SIMD: cycles per instruction and SIMD.
//   part 2: workgroups of 12 waves (3 per SIMD); wave 0 of every SIMD runs a reduce sequence (current: masked DPP adds and
//           selects, 15 instructions; S: swaps, 10; D: DPP on both bank bits, 13; none), the other two run packed FMAs.
//           Cycles per round of (one sequence + 2 x 64 packed FMAs); the difference to "none" is what the sequence costs.
// Every sequence is the 6-row form.  Values are not checked here: tests/test_tile_reduce_gpu.py does that on the kernel.
// Build: hipcc --offload-arch=gfx950 -O3 -o swap_issue swap_issue.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1;}}while(0)
typedef float v2f __attribute__((ext_vector_type(2)));

#define R8(M) M M M M M M M M
#define R64(M) R8(R8(M))

// MODE 0 permlane32_swap, 1 permlane16_swap, 2 v_add_f32_dpp, 3 v_cndmask, 4 v_pk_add_f32, 5 v_pk_fma_f32; 64 statements per
// iteration, of three swaps on three register pairs in turn (a swap reads what a swap wrote two instructions before: the two
// wait states that a VALU write needs in front of a swap's read) or of two of the other instructions
template<int MODE, int WPS>
__global__ void __launch_bounds__(256, WPS) stream(const float* __restrict__ in, float* __restrict__ out, int T, unsigned long long* clk){
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  float a = in[gid % 4096], b = in[(gid + 64) % 4096], c = in[(gid + 128) % 4096], d = in[(gid + 192) % 4096];
  float e = a + c, f = b + d;
  v2f p = {a, b}, q = {c, d}, w = {1.0f, 0.999f};
  unsigned long long t0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
  for(int t=0;t<T;t++){
    if constexpr (MODE==0){ R64(asm volatile("v_permlane32_swap_b32 %0, %1\nv_permlane32_swap_b32 %2, %3\nv_permlane32_swap_b32 %4, %5" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f));) }
    else if constexpr (MODE==1){ R64(asm volatile("v_permlane16_swap_b32 %0, %1\nv_permlane16_swap_b32 %2, %3\nv_permlane16_swap_b32 %4, %5" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f));) }
    else if constexpr (MODE==2){ R64(asm volatile("v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf\nv_add_f32_dpp %2, %3, %3 row_ror:8 row_mask:0xf bank_mask:0xf" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));) }
    else if constexpr (MODE==3){ R64(asm volatile("v_cndmask_b32 %0, %1, %0, vcc\nv_cndmask_b32 %2, %3, %2, vcc" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) :: "vcc");) }
    else if constexpr (MODE==4){ R64(asm volatile("v_pk_add_f32 %0, %0, %2\nv_pk_add_f32 %1, %1, %2" : "+v"(p), "+v"(q) : "v"(w));) }
    else { R64(asm volatile("v_pk_fma_f32 %0, %0, %2, %0\nv_pk_fma_f32 %1, %1, %2, %1" : "+v"(p), "+v"(q) : "v"(w));) }
  }
  unsigned long long t1 = __builtin_amdgcn_s_memtime(), rt1 = __builtin_amdgcn_s_memrealtime();
  out[gid] = a + b + c + d + e + f + p.x + p.y + q.x + q.y;
  if(threadIdx.x==0 && blockIdx.x==0){ clk[0]=t1-t0; clk[1]=rt1-rt0; }
}

// the 6-row reduce sequences on six accumulators x0..x5 (in place; values are meaningless after the first round)
#define SEQ_CUR \
  asm volatile("s_nop 1\n" \
    "v_add_f32_dpp %6, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n" \
    "v_add_f32_dpp %7, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n" \
    "v_add_f32_dpp %8, %2, %2 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n" \
    "v_add_f32_dpp %9, %3, %3 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n" \
    "v_add_f32_dpp %6, %4, %4 row_half_mirror row_mask:0xf bank_mask:0xa\n" \
    "v_add_f32_dpp %7, %5, %5 row_half_mirror row_mask:0xf bank_mask:0xa\n" \
    "v_cndmask_b32 %0, %6, %8, vcc\n v_cndmask_b32 %1, %8, %6, vcc\n" \
    "v_cndmask_b32 %2, %7, %9, vcc\n v_cndmask_b32 %3, %9, %7, vcc\n" \
    "s_nop 1\n" \
    "v_add_f32_dpp %0, %1, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n" \
    "v_add_f32_dpp %2, %3, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n" \
    "v_cndmask_b32 %4, %0, %2, s[2:3]\n v_cndmask_b32 %5, %2, %0, s[2:3]\n" \
    "s_nop 1\n" \
    "v_add_f32_dpp %0, %5, %4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n" \
    : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "=&v"(n0), "=&v"(n1), "=&v"(n2), "=&v"(n3) :: "vcc", "s2", "s3");
#define SEQ_S \
  asm volatile("s_nop 1\n" \
    "v_permlane32_swap_b32 %0, %2\n v_permlane32_swap_b32 %1, %3\n v_permlane32_swap_b32 %4, %5\n" \
    : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5)); \
  { v2f ab = {x0, x1}, cd = {x2, x3}; asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(ab) : "v"(cd)); \
    asm volatile("v_add_f32 %0, %0, %1" : "+v"(x4) : "v"(x5)); x0 = ab.x; x1 = ab.y; } \
  asm volatile("s_nop 1\n v_permlane16_swap_b32 %0, %2\n v_permlane16_swap_b32 %1, %3" : "+v"(x0), "+v"(x1), "+v"(x4), "+v"(x5)); \
  { v2f ab = {x0, x1}, cd = {x4, x5}; asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(ab) : "v"(cd)); x0 = ab.x; x1 = ab.y; } \
  asm volatile("s_nop 1\n" \
    "v_add_f32_dpp %2, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n" \
    "v_add_f32_dpp %2, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xc\n" : "+v"(x0), "+v"(x1), "=&v"(n0));  x2 = n0;
#define SEQ_D \
  asm volatile("s_nop 1\n" \
    "v_add_f32_dpp %6, %0, %0 row_shl:4 row_mask:0xf bank_mask:0x5\n v_add_f32_dpp %6, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xa\n" \
    "v_add_f32_dpp %7, %1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n v_add_f32_dpp %7, %3, %3 row_shr:4 row_mask:0xf bank_mask:0xa\n" \
    "v_add_f32_dpp %8, %4, %4 row_shl:4 row_mask:0xf bank_mask:0x5\n v_add_f32_dpp %8, %5, %5 row_shr:4 row_mask:0xf bank_mask:0xa\n" \
    "s_nop 1\n" \
    "v_add_f32_dpp %0, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xf\n v_add_f32_dpp %0, %8, %8 row_ror:8 row_mask:0xf bank_mask:0xc\n" \
    "v_add_f32_dpp %1, %7, %7 row_ror:8 row_mask:0xf bank_mask:0xf\n v_add_f32_dpp %1, %7, %7 row_ror:8 row_mask:0xf bank_mask:0xc\n" \
    "v_cndmask_b32 %2, %0, %1, vcc\n v_cndmask_b32 %3, %1, %0, vcc\n" \
    "s_nop 1\n" \
    "v_add_f32_dpp %4, %3, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n" \
    : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(n0), "+v"(n1), "+v"(n2) :: "vcc");

// SEQ 0 none, 1 current, 2 S, 3 D.  12 waves per workgroup, one workgroup per CU: waves 0-3 (one per SIMD) run the sequence,
// waves 4-11 the packed FMAs; ROUNDS per iteration.
template<int SEQ>
__global__ void __launch_bounds__(768, 1) mix(const float* __restrict__ in, float* __restrict__ out, int T, unsigned long long* clk){
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float x0 = in[gid % 4096], x1 = in[(gid + 1) % 4096], x2 = in[(gid + 2) % 4096], x3 = in[(gid + 3) % 4096], x4 = in[(gid + 4) % 4096], x5 = in[(gid + 5) % 4096];
  float n0 = 0, n1 = 0, n2 = 0, n3 = 0;
  v2f p = {x0, x1}, q = {x2, x3}, w = {1.0f, 0.999f};
  unsigned long long t0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
  if (wave < 4) {
    for(int t=0;t<T;t++){
      if constexpr (SEQ==1){ R8(SEQ_CUR) } else if constexpr (SEQ==2){ R8(SEQ_S) } else if constexpr (SEQ==3){ R8(SEQ_D) }
      __builtin_amdgcn_s_barrier();
    }
  } else {
    for(int t=0;t<T;t++){
      R8(R8(asm volatile("v_pk_fma_f32 %0, %0, %2, %0\nv_pk_fma_f32 %1, %1, %2, %1\nv_pk_fma_f32 %0, %0, %2, %0\nv_pk_fma_f32 %1, %1, %2, %1\n"
                         "v_pk_fma_f32 %0, %0, %2, %0\nv_pk_fma_f32 %1, %1, %2, %1\nv_pk_fma_f32 %0, %0, %2, %0\nv_pk_fma_f32 %1, %1, %2, %1" : "+v"(p), "+v"(q) : "v"(w));))
      __builtin_amdgcn_s_barrier();
    }
  }
  unsigned long long t1 = __builtin_amdgcn_s_memtime(), rt1 = __builtin_amdgcn_s_memrealtime();
  out[gid] = x0 + x1 + x2 + x3 + x4 + x5 + n0 + n1 + n2 + n3 + p.x + p.y + q.x + q.y;
  if(threadIdx.x==0 && blockIdx.x==0){ clk[0]=t1-t0; clk[1]=rt1-rt0; }
}

template<int MODE, int WPS> int run_stream(const char* name, const float* din, float* dout, unsigned long long* dclk){
  const int T = 2000; const int blocks = 256*WPS;
  stream<MODE,WPS><<<blocks,256>>>(din,dout,T/10,dclk); CK(hipDeviceSynchronize());
  for (int rep = 0; rep < 3; rep++) {
    stream<MODE,WPS><<<blocks,256>>>(din,dout,T,dclk); CK(hipDeviceSynchronize());
    unsigned long long h[2]; CK(hipMemcpy(h,dclk,16,hipMemcpyDeviceToHost));
    double ghz = (double)h[0]/(double)h[1]*0.1;
    printf("%-22s wps=%d rep=%d clk=%.2f GHz  cycles/instr/SIMD=%.2f\n", name, WPS, rep, ghz, (double)h[0] / ((double)WPS * (MODE < 2 ? 192.0 : 128.0) * T));
  }
  return 0;
}
template<int SEQ> int run_mix(const char* name, int ninstr, const float* din, float* dout, unsigned long long* dclk, double* cyc){
  const int T = 2000;
  mix<SEQ><<<256,768>>>(din,dout,T/10,dclk); CK(hipDeviceSynchronize());
  for (int rep = 0; rep < 3; rep++) {
    mix<SEQ><<<256,768>>>(din,dout,T,dclk); CK(hipDeviceSynchronize());
    unsigned long long h[2]; CK(hipMemcpy(h,dclk,16,hipMemcpyDeviceToHost));
    cyc[rep] = (double)h[0] / (8.0 * T);      // per round: one sequence + 2 x 64 packed FMAs on every SIMD
    printf("%-22s rep=%d cycles/round/SIMD=%.1f  (sequence of %d vector instructions)\n", name, rep, cyc[rep], ninstr);
  }
  return 0;
}

#define STREAMS(WPS) \
  if(run_stream<0,WPS>("v_permlane32_swap", din,dout,dclk)) return 1; \
  if(run_stream<1,WPS>("v_permlane16_swap", din,dout,dclk)) return 1; \
  if(run_stream<2,WPS>("v_add_f32_dpp", din,dout,dclk)) return 1; \
  if(run_stream<3,WPS>("v_cndmask_b32", din,dout,dclk)) return 1; \
  if(run_stream<4,WPS>("v_pk_add_f32", din,dout,dclk)) return 1; \
  if(run_stream<5,WPS>("v_pk_fma_f32", din,dout,dclk)) return 1;

int main(){
  float *din,*dout; unsigned long long* dclk;
  std::vector<float> h(4096);
  for(size_t i=0;i<h.size();i++) h[i] = ((i*2654435761u)%1000)/1000.f*0.01f-0.005f;
  CK(hipMalloc(&din,h.size()*4)); CK(hipMalloc(&dout,(size_t)256*768*4)); CK(hipMalloc(&dclk,16));
  CK(hipMemcpy(din,h.data(),h.size()*4,hipMemcpyHostToDevice));
  STREAMS(1)
  STREAMS(2)
  STREAMS(3)
  double none[3], cur[3], s[3], d[3];
  if(run_mix<0>("none", 0, din,dout,dclk,none)) return 1;
  if(run_mix<1>("current (DPP+select)", 15, din,dout,dclk,cur)) return 1;
  if(run_mix<2>("S (swaps)", 10, din,dout,dclk,s)) return 1;
  if(run_mix<3>("D (DPP, both banks)", 13, din,dout,dclk,d)) return 1;
  for (int r = 0; r < 3; r++)
    printf("rep=%d cost of one sequence, cycles/SIMD: current %.1f  S %.1f  D %.1f\n", r, cur[r]-none[r], s[r]-none[r], d[r]-none[r]);
  return 0;
}
