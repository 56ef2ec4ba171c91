// The two waveform-tail kernels of istft_pqmf.hip, which includes this file twice: once as they have always been
// (MBV_ISTFT_POOL 0: istft_pqmf_kernel / istft_single_kernel, one-shot and RANGED), once with the range and the
// destination of every row read from a table (MBV_ISTFT_POOL 1: istft_pqmf_pool_kernel / istft_single_pool_kernel,
// mbv_decode_chunks).  Text, not a shared __device__ function: hipcc schedules an inlined body differently, and the
// instruction streams of the first set are pinned (scripts/istft_disasm.py, tests/test_stream_plan.py).  Every
// sample is computed by the same source lines either way; only where a row's range comes from and where its
// samples go differ.
// POOL: row b is a window of pool[b].len z-frames inside a launch laid out for a.Tp (a.F), handled like a row of
// the ragged decode of that length; units [keep_lo, keep_hi) of it are kept, unit u at pool[b].o + 4 (u - keep_lo).
#if MBV_ISTFT_POOL
template <int TM, int NTHREADS, bool FIXED, bool FAST>
__global__ __launch_bounds__(NTHREADS, (2048 / NTHREADS) * (NTHREADS / 256)) void istft_pqmf_pool_kernel(const IstftArgs a, const float* __restrict__ taps,
                                                              int tiles_per_utt, int total_tiles, const PoolRow* __restrict__ pool) {
  constexpr bool PRE = true, POLAR = false, RANGED = true;
#else
template <int TM, int NTHREADS, bool FIXED, bool FAST, bool PRE, bool POLAR, bool RANGED = false>
__global__ __launch_bounds__(NTHREADS, (2048 / NTHREADS) * (NTHREADS / 256)) void istft_pqmf_kernel(const IstftArgs a, const float* __restrict__ taps,
                                                              int tiles_per_utt, int total_tiles, const IstftRange rg) {
#endif
  constexpr int NF = TM / 4 + 7;          // frames a tile touches per band
  constexpr int NFS = ((NF + 31) / 32) * 32 + 8;   // LDS frame stride, == 8 (mod 32): conflict-free phase B
  constexpr int YL = TM + 16;             // sub-band samples incl. PQMF halo
  constexpr int NROW = 4;                 // rows of the phase-B product (U_1..U_4 or y_band)
  static_assert(4 * NF <= NTHREADS, "one lane per (band, frame)");
  static_assert(YL <= NTHREADS, "one lane per sub-band time index");
  static_assert(NROW * YL <= 4 * 16 * NFS, "phase-B product aliases the frame buffer");
  __shared__ __attribute__((aligned(16))) float fr[4 * 16 * NFS];
  float* const prod = fr;                 // reused after the frames are consumed

  // XCD-aware tile order: workgroups with equal (id % 8) share an L2; give each
  // of the 8 groups a contiguous run of tiles so halo rows are re-read on-die.
  int tile;
  {
    const int bid = blockIdx.x, q = total_tiles / 8, r = total_tiles % 8, x = bid % 8;
    tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
  }
  const int b = tile / tiles_per_utt;
#if MBV_ISTFT_POOL
  const PoolRow pr = pool[b];
  const IstftRange rg{pr.keep_lo, pr.keep_hi, 0, nullptr, nullptr};       // this row's own range
#endif
  const int m0 = ((tile % tiles_per_utt) + (RANGED ? rg.keep_lo / TM : 0)) * TM;
  // opt-in trimmed decode: sub-band samples at and beyond 64 * trim_lens[b] belong to no valid frame; a tile
  // wholly beyond is not computed (the caller zero-filled o), the tile across the boundary stores zeros there
  const int m_valid = a.trim_lens ? 64 * a.trim_lens[b] : 0x7fffffff;
  if (m0 >= m_valid) return;
  const int Tp = a.Tp;
  const int F = 16 * Tp + 1;
  const int M = 64 * Tp;                  // sub-band samples per band
  // frames / samples that exist for this row (RANGED + row_lens: the row's own; F and M stay the strides)
  int Fe = F, Me = M, orow = b;
#if MBV_ISTFT_POOL
  Fe = 16 * pr.len + 1; Me = 64 * pr.len; (void)orow;
  if (m0 >= Me || m0 >= rg.keep_hi) return;       // (the grid is sized for the longest chunk of the run)
#else
  if constexpr (RANGED) {
    if (rg.row_lens) {
      const int len = rg.row_lens[b];
      Fe = 16 * len + 1; Me = 64 * len;
      if (m0 >= Me) return;
    }
    if (rg.row_map) orow = rg.row_map[b];
  }
#endif
  const int tid = threadIdx.x;
  const int f_lo = m0 / 4 - 3;
  // raw buffer descriptors (stride 0, byte range of the whole tensor; launcher checks < 4 GiB)
  constexpr int kRsrcFlags = 0x00020000;
  const __amdgpu_buffer_rsrc_t xrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x_post), 0, POLAR ? 0 : a.B * 72 * F * 4, kRsrcFlags);
  const __amdgpu_buffer_rsrc_t srsrc =
      __builtin_amdgcn_make_buffer_rsrc(a.spec, 0, a.spec ? a.B * 36 * F * 4 : 0, kRsrcFlags);
  const __amdgpu_buffer_rsrc_t prsrc =
      __builtin_amdgcn_make_buffer_rsrc(a.phase, 0, a.phase ? a.B * 36 * F * 4 : 0, kRsrcFlags);

  // ---------------- phase A: frames --------------------------------------
  if (tid < 4 * NF) {
    const int band = tid / NF, fl = tid % NF;
    const int f = f_lo + fl;
    float out[16];
    if (f >= 0 && f < Fe) {
      float re[9], im[9];
      if constexpr (POLAR) {
        // input = (spec, phase) tensors [B, 4, 9, F] (chunked decode: cross-faded spectrograms)
        const int so = ((b * 4 + band) * 9 * F + f) * 4;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const float mag = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srsrc, so, k * F * 4, 0));
          const float ph = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(prsrc, so, k * F * 4, 0));
          polar_in<FAST>(mag, ph, re[k], im[k], k != 0 && k != 8);
        }
      } else {
        // buffer loads: one 32-bit lane offset, the 18 channel strides ride in scalar registers
        const int voff = ((b * 72 + band * 18) * F + f) * 4;
        float xin[18];
#pragma unroll
        for (int k = 0; k < 18; ++k)
          xin[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, voff, k * F * 4, 0));
        // frame f is owned (for the spec/phase outputs) by the tile holding sample 4f
        // (RANGED: a.spec / a.phase are null at run time.  The stores stay in the code, so that the values they would
        // store keep the uses, and with them the fused multiply-adds, of the one-shot kernel: bitwise the same samples.)
        const bool own = (4 * f >= m0 && 4 * f < m0 + TM) || (f == F - 1 && m0 + TM >= M);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          float mag, ph;
          polar<FAST, PRE>(xin[k], xin[9 + k], mag, ph, re[k], im[k], k != 0 && k != 8);
          if (own) {
            const int so = ((b * 4 + band) * 9 * F + f) * 4;
            if (a.spec) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, mag), srsrc, so, k * F * 4, 0);
            if (a.phase) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, ph), prsrc, so, k * F * 4, 0);
          }
        }
      }
      irfft16_hann(re, im, out);
    } else {
#pragma unroll
      for (int n = 0; n < 16; ++n) out[n] = 0.f;
    }
#pragma unroll
    for (int n = 0; n < 16; ++n) fr[(band * 16 + n) * NFS + fl] = out[n];
  }
  __syncthreads();

  // ---------------- phase B: overlap-add + envelope (+ modulation) ---------
  float rowv[NROW];
  {
    const int u = tid;                    // m = m0 - 8 + u
    const int q = u >> 2, r = u & 3;      // quad f' = m0/4 - 2 + q ; frames f'-1 .. f'+2
    const int m = m0 - 8 + u;
    const int fp = m0 / 4 - 2 + q;
    float y[4] = {0.f, 0.f, 0.f, 0.f};
    if (u < YL && m >= 0 && m < Me) {
      float env;
      if (fp - 1 >= 0 && fp + 2 < Fe) {
        env = 1.5f;                        // sum of squared hann over 4 overlapping frames
      } else {
        env = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int f = fp - 1 + g;
          env += (f >= 0 && f < Fe) ? WSQ16[12 - 4 * g + r] : 0.f;
        }
      }
      const float renv = 1.f / env;          // one division per lane (torch.istft divides per sample)
#pragma unroll
      for (int band = 0; band < 4; ++band) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g)      // frame f'-1+g contributes its sample n = 12 - 4g + r
          s += fr[(band * 16 + 12 - 4 * g + r) * NFS + q + g];
        y[band] = s * renv;
      }
      if (a.o_mb && u >= 8 && u < TM + 8) {          // (RANGED: null at run time, kept in the code as above)          // owned samples m0 .. m0+TM-1
        if (!a.multistream) {
#pragma unroll
          for (int band = 0; band < 4; ++band) a.o_mb[((int64_t)b * 4 + band) * M + m] = y[band];
        } else {                                       // zero-stuffed x4, gain 4 (models.py:463)
          typedef float f4v __attribute__((ext_vector_type(4)));
#pragma unroll
          for (int band = 0; band < 4; ++band) {
            f4v v = {4.f * y[band], 0.f, 0.f, 0.f};
            f4v* dst = reinterpret_cast<f4v*>(a.o_mb + ((int64_t)b * 4 + band) * 4 * M + 4 * (int64_t)m);
            *dst = v;
          }
        }
      }
    }
    if constexpr (FIXED) {
      // Of the 8 modulation phases only 4 are distinct: U_0 = U_1, U_5 = -U_4, U_6 = -U_3,
      // U_7 = -U_2 (theta_k(q) is symmetric about q = 0.5 and anti-symmetric about q = 4.5).
      // Row r holds U_{r+1}; the signs are folded into the tap constants of phase C.
#pragma unroll
      for (int r = 0; r < 4; ++r)
        rowv[r] = PQMF_C[r + 1] * y[0] + PQMF_C[8 + r + 1] * y[1] + PQMF_C[16 + r + 1] * y[2] +
                  PQMF_C[24 + r + 1] * y[3];
    } else {
#pragma unroll
      for (int band = 0; band < 4; ++band) rowv[band] = y[band];
    }
  }
  __syncthreads();                        // every lane has consumed its frames: reuse the buffer
  if (tid < YL) {
#pragma unroll
    for (int k = 0; k < NROW; ++k) prod[k * YL + tid] = rowv[k];
  }
  __syncthreads();

  // ---------------- phase C: polyphase synthesis filter --------------------
  if (tid < TM) {
    const int m = m0 + tid;
    if (m < Me) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (FIXED) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int j = 3 - p + 4 * i;           // tap index; y index m - 7 + i
            if (j <= 62) {
              constexpr int ROW[8] = {0, 0, 1, 2, 3, 3, 2, 1};          // U_q -> stored row
              constexpr float SGN[8] = {1.f, 1.f, 1.f, 1.f, 1.f, -1.f, -1.f, -1.f};
              acc[p] = fmaf(PQMF_G[j] * SGN[j & 7], prod[ROW[j & 7] * YL + tid + 1 + i], acc[p]);
            }
          }
        }
      } else {
#pragma unroll
        for (int band = 0; band < 4; ++band) {
          const float* yb = &prod[band * YL + tid + 1];        // y[m - 7 + i]
          const float* hb = taps + band * 64;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float yv = yb[i];
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[p] = fmaf(hb[p * 16 + i], yv, acc[p]);
          }
        }
      }
#if MBV_ISTFT_POOL
      if (m >= rg.keep_lo && m < rg.keep_hi)
        *reinterpret_cast<float4*>(pr.o + 4 * (int64_t)(m - rg.keep_lo)) = make_float4(acc[0], acc[1], acc[2], acc[3]);
#else
      if constexpr (RANGED) {
        if (m >= rg.keep_lo && m < rg.keep_hi)
          *reinterpret_cast<float4*>(a.o + (int64_t)orow * rg.o_row_stride + 4 * (int64_t)(m - rg.keep_lo)) =
              make_float4(acc[0], acc[1], acc[2], acc[3]);
      } else {
        *reinterpret_cast<float4*>(a.o + (int64_t)b * 4 * M + 4 * (int64_t)m) =
            m < m_valid ? make_float4(acc[0], acc[1], acc[2], acc[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#endif
    }
  }
}

// the single-band tail (described above launch_istft_single in istft_pqmf.hip)
#if MBV_ISTFT_POOL
template <bool FAST>
__global__ __launch_bounds__(256) void istft_single_pool_kernel(const IstftSbArgs a, int tiles_per_utt, const PoolRow* __restrict__ pool) {
  constexpr bool PRE = true, POLAR = false, RANGED = true;
#else
template <bool FAST, bool PRE, bool POLAR, bool RANGED = false>
__global__ __launch_bounds__(256) void istft_single_kernel(const IstftSbArgs a, int tiles_per_utt, const IstftRange rg) {
#endif
  constexpr int QPB = 252;                 // output quads per workgroup
  constexpr int NFS = 256;
  __shared__ float fr[16 * NFS];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / tiles_per_utt;
#if MBV_ISTFT_POOL
  const PoolRow pr = pool[b];
  const IstftRange rg{pr.keep_lo, pr.keep_hi, 0, nullptr, nullptr};
#endif
  const int q0 = ((blockIdx.x % tiles_per_utt) + (RANGED ? rg.keep_lo / QPB : 0)) * QPB;
  const int F = a.F;
  // frames that exist for this row (RANGED + row_lens: 64 len_b + 1, see istft_pqmf_kernel; F stays the stride)
  int Fe = F, orow = b;
#if MBV_ISTFT_POOL
  Fe = 64 * pr.len + 1; (void)orow;
  if (q0 >= Fe - 1 || q0 >= rg.keep_hi) return;
#else
  if constexpr (RANGED) {
    if (rg.row_lens) {
      Fe = 64 * rg.row_lens[b] + 1;
      if (q0 >= Fe - 1) return;
    }
    if (rg.row_map) orow = rg.row_map[b];
  }
#endif
  const int nquads = Fe - 1;               // 4 (F-1) output samples

  {
    const int f = q0 - 1 + tid;
    float out[16];
    if (tid < QPB + 3 && f >= 0 && f < Fe) {
      float re[9], im[9];
      if constexpr (POLAR) {
#pragma unroll
        for (int k = 0; k < 9; ++k)
          polar_in<FAST>(a.spec[((int64_t)b * 9 + k) * F + f], a.phase[((int64_t)b * 9 + k) * F + f],
                         re[k], im[k], k != 0 && k != 8);
      } else {
        const float* xp = a.x_post + (int64_t)b * 18 * F + f;
        float xin[18];
#pragma unroll
        for (int k = 0; k < 18; ++k) xin[k] = xp[(int64_t)k * F];
        const bool own = f >= q0 && (f < q0 + QPB || f == F - 1);     // (RANGED: spec / phase null, see istft_pqmf_kernel)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          float mag, ph;
          polar<FAST, PRE>(xin[k], xin[9 + k], mag, ph, re[k], im[k], k != 0 && k != 8);
          if (own) {
            if (a.spec) a.spec[((int64_t)b * 9 + k) * F + f] = mag;
            if (a.phase) a.phase[((int64_t)b * 9 + k) * F + f] = ph;
          }
        }
      }
      irfft16_hann(re, im, out);
    } else {
#pragma unroll
      for (int n = 0; n < 16; ++n) out[n] = 0.f;
    }
#pragma unroll
    for (int n = 0; n < 16; ++n) fr[n * NFS + tid] = out[n];
  }
  __syncthreads();
  const int fp = q0 + tid;                 // quad f': samples 4 f' + r from frames f'-1 .. f'+2
  if (tid < QPB && fp < nquads) {
    float y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sacc = 0.f, env = 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int f = fp - 1 + g;
        sacc += fr[(12 - 4 * g + r) * NFS + tid + g];
        env += (f >= 0 && f < Fe) ? HANN16[12 - 4 * g + r] * HANN16[12 - 4 * g + r] : 0.f;
      }
      y[r] = sacc / env;
    }
#if MBV_ISTFT_POOL
    if (fp >= rg.keep_lo && fp < rg.keep_hi)
      *reinterpret_cast<float4*>(pr.o + 4 * (int64_t)(fp - rg.keep_lo)) = make_float4(y[0], y[1], y[2], y[3]);
#else
    if constexpr (RANGED) {
      if (fp >= rg.keep_lo && fp < rg.keep_hi)
        *reinterpret_cast<float4*>(a.o + (int64_t)orow * rg.o_row_stride + 4 * (int64_t)(fp - rg.keep_lo)) =
            make_float4(y[0], y[1], y[2], y[3]);
    } else {
      *reinterpret_cast<float4*>(a.o + (int64_t)b * 4 * nquads + 4 * (int64_t)fp) =
          make_float4(y[0], y[1], y[2], y[3]);
    }
#endif
  }
}
