// Kernels of the ResNet bottleneck backbone (eval forward): everything that is not a 1x1 convolution.  The 1x1 convolutions run on the
// three-piece split-precision GEMM (axvs_gemm_nt.h) with the folded BatchNorm as their bias.  Maps travel channels-last from the stem's
// output to the last block: rows [N][h][w][C] fp32.  Every BatchNorm arrives folded (float64, by the caller) into the weights and a bias.
//
//   rn_pack_stem_kernel   the folded stem weight [147][Cs] fp32 -> its three bf16 pieces in the fragment order rn_stem_kernel reads
//   rn_stem_kernel        image [N, 3, H, W] -> rows [N][hp][wp][Cs]: 7x7 / stride 2 / padding 3 convolution (the zeros come from the
//                         index test; three-piece MFMA, K padded to 160) + bias + ReLU + 3x3 / stride 2 / padding 1 max pool in ONE
//                         launch; the stride-2 map lives in LDS only
//   rn_gather2_kernel     rows [N][h][w][C] -> rows [N][ceil(h/2)][ceil(w/2)][C], pixel (2y, 2x): what a stride-2 1x1 convolution reads
//   rn_pack_w3_kernel     a folded 3x3 weight [C][9][C] fp32 -> its three bf16 pieces in the fragment order rn_conv3_kernel reads
//   rn_conv3_kernel       3x3 convolution (stride 1 / 2, dilation = padding 1 / 2, C -> C) + bias + ReLU: see there
// and rows [N*h*w][C] -> [N, C, h, w] for the outputs: rows_to_nchw() (axvs_layout.h).
// No kernel waits for another workgroup and none adds floating-point numbers atomically: equal inputs give equal bits, and a frame's
// bits do not depend on the frames stacked beside it.
#pragma once
#include <hip/hip_runtime.h>

#include "axvs_common.h"
#include "axvs_gemm_nt.h"

namespace axvs {

// ---- the stem --------------------------------------------------------------------------------------------------------------------------
// A workgroup owns 8 x 7 pooled pixels = the 17 x 15 convolution pixels under them (255 of the 256 rows of sixteen 16-pixel m-tiles, four
// per wave) = a 39 x 35 image patch per colour in LDS (fp32).  The contraction (K = 147, padded to 160 = five 32-wide steps) runs on
// v_mfma_f32_16x16x32_bf16 with three bf16 pieces per operand and the six products hh, hm, mh, mm, hl, lh per accumulator, as in
// tr_gemm_nt_kernel<3>.  Per pass of up to 64 output channels (four n-tiles; R-50's stem is one pass) and per step a lane gathers the eight
// patch values of its (pixel, k-group) -- k = (colour, ky, kx), zeros past 147 -- and splits them once for all four n-tiles; the weights
// are pre-split at pack time (rn_pack_stem_kernel) into [Cs / 16 n-tiles][5 steps][3 pieces][64 lanes][8], one contiguous KiB per
// fragment, and read from L2.  relu(sum + bias) goes to the LDS tile [255][64] (pitch 68 floats: the sixteen pixels of a store fall on
// different banks), and after a barrier 224 threads take the 3x3 maxima of four channels per n-tile each and write them.  A convolution
// pixel outside the stride-2 map is written as 0: every value behind the ReLU is >= 0 and every pooling window holds at least one pixel
// of the map, so the pool's padding value (-inf in the reference) never decides a maximum.  An n-tile past Cs reads n-tile 0's weights,
// is multiplied like the others (no branch in the step loop) and is not written.
constexpr int kRnStemPH = 8, kRnStemPW = 7;                                   // pooled pixels per workgroup
constexpr int kRnStemCH = 2 * kRnStemPH + 1, kRnStemCW = 2 * kRnStemPW + 1;   // 17 x 15 convolution pixels
constexpr int kRnStemIH = 2 * kRnStemCH + 5, kRnStemIW = 2 * kRnStemCW + 5;   // 39 x 35 image pixels
constexpr int kRnStemIP = kRnStemIW + 1;                                      // LDS pitch of a patch row
constexpr int kRnStemNT = 4, kRnStemCC = 16 * kRnStemNT;                      // n-tiles / output channels per pass
constexpr int kRnStemCP = kRnStemCC + 4;                                      // LDS pitch of a convolution pixel's channels
constexpr int kRnStemK = 147, kRnStemSteps = 5;                               // the contraction, and its 32-wide steps
constexpr int kRnStemPatch = 3 * kRnStemIH * kRnStemIP;                       // floats
constexpr int kRnStemLds = (kRnStemPatch + kRnStemCH * kRnStemCW * kRnStemCP) * (int)sizeof(float);
__host__ __device__ inline size_t rn_stem_w_elems(int Cs) { return (size_t)(Cs / 16) * kRnStemSteps * 3 * 512; }      // u16 of the packed stem weight

// w [147][Cs] ((colour, ky, kx) major, output channel fastest) fp32 -> the packed pieces; one thread per (n-tile, step, lane)
__global__ __launch_bounds__(256) void rn_pack_stem_kernel(const float* __restrict__ w, u16* __restrict__ dst, int Cs, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int lane = (int)(i & 63), fi = lane & 15, fg = lane >> 4;
  const size_t frag = i >> 6;                           // n-tile * steps + step
  const int step = (int)(frag % kRnStemSteps), nt = (int)(frag / kRnStemSteps);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = step * 32 + fg * 8 + e;
    v[e] = k < kRnStemK ? w[(size_t)k * Cs + nt * 16 + fi] : 0.f;
  }
  u16x8 p[3];
  tr::split_n<3>(float4{v[0], v[1], v[2], v[3]}, float4{v[4], v[5], v[6], v[7]}, p);
#pragma unroll
  for (int s = 0; s < 3; ++s) *reinterpret_cast<u16x8*>(dst + (frag * 3 + s) * 512 + lane * 8) = p[s];
}

// grid (ceil(wp / 7), ceil(hp / 8), N); dynamic LDS kRnStemLds
__global__ __launch_bounds__(256) void rn_stem_kernel(const float* __restrict__ image, const u16* __restrict__ wpk, const float* __restrict__ bias,
                                                      float* __restrict__ out, int Cs, int H, int W, int hc, int wc, int hp, int wp) {
  extern __shared__ __attribute__((aligned(16))) char rn_stem_smem[];
  float* const patch = reinterpret_cast<float*>(rn_stem_smem);      // [3][39][36]
  float* const conv = patch + kRnStemPatch;                          // [255][68]
  const int tid = threadIdx.x, n = blockIdx.z, lane = tid & 63, wave = tid >> 6, fi = lane & 15, fg = lane >> 4;
  const int py0 = blockIdx.y * kRnStemPH, px0 = blockIdx.x * kRnStemPW;
  const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;            // first convolution pixel of the tile (may be -1)
  const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;            // first image pixel of the patch
  const float* img = image + (size_t)n * 3 * H * W;
  for (int i = tid; i < 3 * kRnStemIH * kRnStemIW; i += 256) {
    const int c = i / (kRnStemIH * kRnStemIW), r = i % (kRnStemIH * kRnStemIW), y = r / kRnStemIW, x = r % kRnStemIW;
    const int iy = iy0 + y, ix = ix0 + x;
    patch[(c * kRnStemIH + y) * kRnStemIP + x] = iy >= 0 && iy < H && ix >= 0 && ix < W ? img[((size_t)c * H + iy) * W + ix] : 0.f;
  }
  __syncthreads();
  // this lane's pixel of each of the wave's four m-tiles: its patch offset, whether it exists, whether it lies in the stride-2 map
  int poff[4];
  bool has_px[4], in_map[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int m = wave * 64 + mt * 16 + fi;
    has_px[mt] = m < kRnStemCH * kRnStemCW;
    const int ly = has_px[mt] ? m / kRnStemCW : 0, lx = has_px[mt] ? m % kRnStemCW : 0;
    poff[mt] = 2 * ly * kRnStemIP + 2 * lx;
    in_map[mt] = has_px[mt] && cy0 + ly >= 0 && cy0 + ly < hc && cx0 + lx >= 0 && cx0 + lx < wc;
  }
  // the pool's side: thread -> (pooled pixel, four channels of each n-tile)
  const int pp = tid >> 2, pq = tid & 3, ply = pp / kRnStemPW, plx = pp % kRnStemPW;
  const bool pool_ok = pp < kRnStemPH * kRnStemPW && py0 + ply < hp && px0 + plx < wp;
  constexpr int kPieceA[6] = {0, 1, 0, 1, 2, 0}, kPieceB[6] = {0, 0, 1, 1, 0, 2};      // (pixel piece, weight piece) of product p
  for (int c0 = 0; c0 < Cs; c0 += kRnStemCC) {
    const u16* wnt[kRnStemNT];
#pragma unroll
    for (int nt = 0; nt < kRnStemNT; ++nt) {
      const int tile = c0 / 16 + nt;
      wnt[nt] = wpk + (size_t)(tile * 16 < Cs ? tile : 0) * kRnStemSteps * 3 * 512 + lane * 8;
    }
    f32x4 acc[4][kRnStemNT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < kRnStemNT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int step = 0; step < kRnStemSteps; ++step) {
      u16x8 bf[kRnStemNT][3];
#pragma unroll
      for (int nt = 0; nt < kRnStemNT; ++nt)
#pragma unroll
        for (int s = 0; s < 3; ++s) bf[nt][s] = *reinterpret_cast<const u16x8*>(wnt[nt] + (step * 3 + s) * 512);
      int koff[8];                      // patch offset of k = (colour, ky, kx); a k past 147 reads offset 0 and counts as zero
      bool kok[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = step * 32 + fg * 8 + e, c = k / 49, r = k - 49 * c, ky = r / 7, kx = r - 7 * ky;
        kok[e] = k < kRnStemK;
        koff[e] = kok[e] ? (c * kRnStemIH + ky) * kRnStemIP + kx : 0;
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = patch[poff[mt] + koff[e]];
          v[e] = kok[e] ? t : 0.f;
        }
        u16x8 af[3];
        tr::split_n<3>(float4{v[0], v[1], v[2], v[3]}, float4{v[4], v[5], v[6], v[7]}, af);
#pragma unroll
        for (int pr = 0; pr < 6; ++pr)
#pragma unroll
          for (int nt = 0; nt < kRnStemNT; ++nt)
            acc[mt][nt] = H16<true>::mfma(bf[nt][kPieceB[pr]], af[kPieceA[pr]], acc[mt][nt]);      // D[oc = 4 fg + r][pixel = fi]
      }
    }
#pragma unroll
    for (int nt = 0; nt < kRnStemNT; ++nt) {
      const int oc = c0 + nt * 16 + 4 * fg;
      if (oc < Cs) {
        const float4 b = *reinterpret_cast<const float4*>(bias + oc);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          if (has_px[mt]) {
            const float4 r = in_map[mt] ? make_float4(fmaxf(acc[mt][nt][0] + b.x, 0.f), fmaxf(acc[mt][nt][1] + b.y, 0.f), fmaxf(acc[mt][nt][2] + b.z, 0.f),
                                                      fmaxf(acc[mt][nt][3] + b.w, 0.f))
                                        : float4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<float4*>(conv + (wave * 64 + mt * 16 + fi) * kRnStemCP + nt * 16 + 4 * fg) = r;
          }
      }
    }
    __syncthreads();
    if (pool_ok) {
#pragma unroll
      for (int nt = 0; nt < kRnStemNT; ++nt) {
        const int oc = c0 + nt * 16 + 4 * pq;
        if (oc < Cs) {
          float4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
              const float4 v = *reinterpret_cast<const float4*>(conv + ((2 * ply + dy) * kRnStemCW + 2 * plx + dx) * kRnStemCP + nt * 16 + 4 * pq);
              m.x = fmaxf(m.x, v.x), m.y = fmaxf(m.y, v.y), m.z = fmaxf(m.z, v.z), m.w = fmaxf(m.w, v.w);
            }
          *reinterpret_cast<float4*>(out + (((size_t)n * hp + py0 + ply) * wp + px0 + plx) * Cs + oc) = m;
        }
      }
    }
    __syncthreads();
  }
}

// ---- rows -> every second pixel of every second row ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rn_gather2_kernel(const float* __restrict__ x, float* __restrict__ y, int C4, int h, int w, int h2, int w2, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;      // (n, y2, x2, float4 of the row)
  if (i >= total) return;
  const int c = (int)(i % C4);
  const size_t p = i / C4;
  const int x2 = (int)(p % w2), y2 = (int)((p / w2) % h2);
  const size_t n = p / ((size_t)w2 * h2);
  reinterpret_cast<float4*>(y)[i] = reinterpret_cast<const float4*>(x)[((n * h + 2 * y2) * w + 2 * x2) * C4 + c];
}

// ---- the 3x3 convolution ---------------------------------------------------------------------------------------------------------------
// An implicit GEMM over (32-channel chunk, tap) on v_mfma_f32_16x16x32_bf16 with three bf16 pieces per operand and the six products hh, hm,
// mh, mm, hl, lh in that order, fp32 accumulation: the products of tr_gemm_nt_kernel<3>.  Unlike that kernel, a (chunk, tap) step sums its
// six products from zero and adds the sum to the running accumulator once: at C = 512 the contraction has 144 steps, and with all 864
// products added to the running sum one by one the result sat at 6.1 and 8.9 x the error of an fp32 convolution (against float64 on
// the 25 x 43 x 512 maps at dilation 1 and 2; with the step sums 1.5 and 1.6 x: profiles/resnet_parity.txt), outside this project's bound
// of 8 x.
//
// Tile: a workgroup of four waves owns TH x 16 output pixels (TH = 8 at stride 1, 4 at stride 2) x BN output channels (128; 64 for C <= 64,
// so that a 64-channel stage keeps all four waves busy, and where 128 would give fewer workgroups than compute units: the launcher
// decides).  Waves are WM x WN; a wave owns TH / WM output rows (one 16-pixel m-tile each) and BN / 16 / WN n-tiles of 16 channels.
// Input: per chunk the halo tile ((TH - 1) S + 1 + 2 d) x (15 S + 1 + 2 d) pixels x 32 channels is loaded ONCE, split into its three pieces
// ONCE and stored to LDS as 64-byte pixel rows per piece (chunk-swizzled with swz_chunk on the pixel's LDS index); all nine taps read their
// fragments from it.  At stride 2 the columns are stored parity-split (even columns, then odd ones), so the 16 pixels of a fragment are
// neighbours in LDS for either stride.  A tap's fragment starts at any pixel index, so the swizzle leaves some 2-way conflicts on the
// ds_read_b128; a wave reads 6 .. 12 such fragments (4 LDS cycles each without a conflict) per 24 .. 96 MFMAs (16 matrix-pipe cycles each),
// so they are left in.
// The chunk's loads for the NEXT chunk are issued (into registers) before the current chunk's nine taps are multiplied; the image is
// single-buffered (two barriers per chunk = per 9 taps: a 512-channel stride-2 halo of three pieces would not fit twice).
// Weights: pre-split at pack time (rn_pack_w3_kernel) into [C/16 n-tiles][C/32 chunks][9 taps][3 pieces][64 lanes][8]: the 1 KiB a wave
// reads as one operand fragment is contiguous and in lane order, and a wave's stream over (chunk, tap) is one contiguous run per n-tile.
// They do NOT go through LDS (the builder's choice against the suggested shape: a tap's weights are read by at most two waves of the
// workgroup, the L1 serves the second, and a (chunk, tap) step gives 48..96 MFMAs = 768..1536 matrix-pipe cycles to cover the load of the
// next step's fragments, which are in flight in registers meanwhile; keeping them out of LDS keeps the nine taps free of barriers).
template <int S, int BN>
struct RnConv3 {
  static constexpr int TH = S == 1 ? 8 : 4, TW = 16;
  static constexpr int WN = S == 1 ? BN / 64 : BN / 32, WM = 4 / WN;
  static constexpr int MT = TH / WM, NT = BN / 16 / WN;
  static constexpr int halo_h(int d) { return (TH - 1) * S + 1 + 2 * d; }
  static constexpr int halo_w(int d) { return (TW - 1) * S + 1 + 2 * d; }
  static constexpr int pitch(int d) { return S == 1 ? halo_w(d) : 2 * ((halo_w(d) + 1) / 2); }      // LDS pixels per halo row
  static constexpr int pixels(int d) { return halo_h(d) * pitch(d); }
  static constexpr int lds(int d) { return 3 * pixels(d) * 64; }                                      // bytes
  static constexpr int kUnits = (halo_h(2) * halo_w(2) * 4 + 255) / 256;      // (pixel, 8-channel group) units per thread, at most
};

constexpr int kRnW3Frag = 512;      // u16 per operand fragment (64 lanes x 8)
__host__ __device__ inline size_t rn_w3_elems(int C) { return (size_t)27 * C * C; }      // u16 of one packed 3x3 weight

// w [C][9][C] (output channel, tap ky*3 + kx, input channel) fp32 -> the packed pieces; one thread per (n-tile, chunk, tap, lane)
__global__ __launch_bounds__(256) void rn_pack_w3_kernel(const float* __restrict__ w, u16* __restrict__ dst, int C, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int lane = (int)(i & 63), fi = lane & 15, fg = lane >> 4;
  const size_t step = i >> 6;                           // (n-tile * chunks + chunk) * 9 + tap
  const int tap = (int)(step % 9), chunk = (int)((step / 9) % (C / 32)), nt = (int)(step / 9 / (C / 32));
  const float* src = w + ((size_t)(nt * 16 + fi) * 9 + tap) * C + chunk * 32 + fg * 8;
  u16x8 p[3];
  tr::split_n<3>(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), p);
#pragma unroll
  for (int s = 0; s < 3; ++s) *reinterpret_cast<u16x8*>(dst + (step * 3 + s) * kRnW3Frag + lane * 8) = p[s];
}

// x rows [N][h][w][C] -> y rows [N][ho][wo][C], ho = ceil(h / S); grid (ceil(wo / 16), ceil(ho / TH), N * ceil(C / BN)); dynamic LDS lds(d)
template <int S, int BN>
__global__ __launch_bounds__(256) void rn_conv3_kernel(const float* __restrict__ x, const u16* __restrict__ wp, const float* __restrict__ bias,
                                                       float* __restrict__ y, int C, int h, int w, int ho, int wo, int d) {
  using K = RnConv3<S, BN>;
  constexpr int TH = K::TH, WN = K::WN, MT = K::MT, NT = K::NT;
  extern __shared__ __attribute__((aligned(16))) char rn_smem[];
  u16* const img = reinterpret_cast<u16*>(rn_smem);      // [3 pieces][pixels][32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, fg = lane >> 4;
  const int wm = wave / WN, wn = wave % WN;
  const int ntile_c = (C + BN - 1) / BN;
  const int n = blockIdx.z / ntile_c, oc0 = (blockIdx.z % ntile_c) * BN;
  const int oy0 = blockIdx.y * TH, ox0 = blockIdx.x * 16;
  const int hh = (TH - 1) * S + 1 + 2 * d, hw = 15 * S + 1 + 2 * d;              // the halo tile
  const int hwh = (hw + 1) / 2, pitch = S == 1 ? hw : 2 * hwh, npix = hh * pitch;
  const int iy0 = oy0 * S - d, ix0 = ox0 * S - d;
  const int nchunks = C / 32, nsteps = nchunks * 9;
  const float* const xn = x + (size_t)n * h * w * C;

  // staging: unit u = tid + 256 i -> (halo pixel u >> 2, 8-channel group u & 3)
  float4 ra[K::kUnits][2];
  const int nunits = hh * hw * 4;
  auto gload = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < K::kUnits; ++i) {
      const int u = tid + 256 * i, px = u >> 2, q = u & 3;
      const int r = px / hw, c = px - r * hw, iy = iy0 + r, ix = ix0 + c;
      const bool ok = u < nunits && iy >= 0 && iy < h && ix >= 0 && ix < w;
      const float* src = xn + ((size_t)(ok ? iy : 0) * w + (ok ? ix : 0)) * C + chunk * 32 + q * 8;
      ra[i][0] = ok ? *reinterpret_cast<const float4*>(src) : float4{0.f, 0.f, 0.f, 0.f};
      ra[i][1] = ok ? *reinterpret_cast<const float4*>(src + 4) : float4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < K::kUnits; ++i) {
      const int u = tid + 256 * i, px = u >> 2, q = u & 3;
      if (u < nunits) {
        const int r = px / hw, c = px - r * hw;
        const int p = r * pitch + (S == 1 ? c : (c & 1) * hwh + (c >> 1));
        u16x8 pc[3];
        tr::split_n<3>(ra[i][0], ra[i][1], pc);
#pragma unroll
        for (int s = 0; s < 3; ++s) *reinterpret_cast<u16x8*>(img + ((size_t)s * npix + p) * 32 + swz_chunk(p, q) * 8) = pc[s];
      }
    }
  };

  // this wave's n-tiles and weight streams.  An n-tile past C (C is no multiple of BN) reads n-tile 0's weights and is multiplied like the
  // others -- a branch per n-tile in the tap loop put every MFMA into a basic block of its own, with the accumulators copied between the
  // two register files around each (5060 v_accvgpr moves in the <1, 128> form against 64 now) -- and is not written.
  bool nt_ok[NT];
  const u16* wnt[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int tile = oc0 / 16 + wn * NT + nt;
    nt_ok[nt] = tile * 16 < C;
    wnt[nt] = wp + (size_t)(nt_ok[nt] ? tile : 0) * nsteps * 3 * kRnW3Frag + lane * 8;
  }
  u16x8 bcur[NT][3], bnxt[NT][3];
  auto wload = [&](int step, u16x8 (&b)[NT][3]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int s = 0; s < 3; ++s) b[nt][s] = *reinterpret_cast<const u16x8*>(wnt[nt] + ((size_t)step * 3 + s) * kRnW3Frag);
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  wload(0, bcur);
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    __syncthreads();            // every wave has left the previous chunk's image
    lstore();
    __syncthreads();
    if (chunk + 1 < nchunks) gload(chunk + 1);
#pragma unroll 1      // (unrolled, the nine taps' fragment loads are hoisted over one another and the kernel spills)
    for (int tap = 0; tap < 9; ++tap) {
      const int step = chunk * 9 + tap, ky = (tap * 11) >> 5, kx = tap - 3 * ky;
      wload(step + 1 < nsteps ? step + 1 : step, bnxt);      // (no branch in the tap loop: the last step loads its own fragments again)
      const int cb = S == 1 ? kx * d : ((kx * d) & 1) * hwh + ((kx * d) >> 1);
      constexpr int kPieceA[6] = {0, 1, 0, 1, 2, 0}, kPieceB[6] = {0, 0, 1, 1, 0, 2};      // (pixel piece, weight piece) of product p
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int p = ((wm * MT + mt) * S + ky * d) * pitch + cb + fi;
        u16x8 af[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) af[s] = *reinterpret_cast<const u16x8*>(img + ((size_t)s * npix + p) * 32 + swz_chunk(p, fg) * 8);
        // the step's six products are summed from zero and reach the accumulator as ONE addition: a rounding of the accumulator is as
        // large as the accumulator, whatever is added, and five of six additions would be spent on the small cross terms
        f32x4 part[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) part[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pr = 0; pr < 6; ++pr)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            part[nt] = H16<true>::mfma(bcur[nt][kPieceB[pr]], af[kPieceA[pr]], part[nt]);      // D[oc = 4 fg + r][pixel = fi]
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] += part[nt];
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int s = 0; s < 3; ++s) bcur[nt][s] = bnxt[nt][s];
    }
  }
  // epilogue: + bias, ReLU; lane -> pixel ox0 + fi of its rows, four channels per n-tile
  const int ox = ox0 + fi;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    if (!nt_ok[nt]) continue;
    const int oc = oc0 + (wn * NT + nt) * 16 + 4 * fg;
    const float4 b = *reinterpret_cast<const float4*>(bias + oc);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int oy = oy0 + wm * MT + mt;
      if (oy < ho && ox < wo)
        *reinterpret_cast<float4*>(y + (((size_t)n * ho + oy) * wo + ox) * C + oc) =
            make_float4(fmaxf(acc[mt][nt][0] + b.x, 0.f), fmaxf(acc[mt][nt][1] + b.y, 0.f), fmaxf(acc[mt][nt][2] + b.z, 0.f), fmaxf(acc[mt][nt][3] + b.w, 0.f));
    }
  }
}

}  // namespace axvs
