// The body of the KV-cached attention kernels for ONE new token per sequence, #included inside attn_decode_kernel<DHS, ROWS> (decode.hip)
// and attn_decode_anc_kernel<DHS> (beam.hip).  Text inclusion, not a __device__ function: a function inlined into the kernels makes the
// compiler schedule and contract the existing kernels' arithmetic differently, and they must stay the instructions they were.
// In scope where it is included: DHS, ROWS (constants), qkv, cache, y, B, n_head, Tmax, pos_arg, pos_dev, and the macro
// ATTN_DECODE_SEQ(t) = the base of the cached (b, head) sequence that holds position t < pos of this wave's row ("seq", the row's own,
// in decode.hip; the ancestor's in beam.hip).
//
// qkv: [B, 3C] bf16 of the new token (q, k already rotated by the QKV GEMM epilogue); y: [B, C] bf16.
// One wave per (b, head).  Appends (k, v) at position pos, attends to positions 0..pos.
// ROWS (ragged sessions): pos_dev is an array, row b sits at its own position pos_dev[b]; a position outside 0 .. Tmax - 1 marks an
// idle slot, whose waves return before they read or write anything (their cache records and y rows keep what they held).  The
// four passes below load only the records t <= pos, so a short row streams its own length, not the batch's.
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= B * n_head) return;
  const int b = item / n_head, h = item - b * n_head;
  const int pos = ROWS ? pos_dev[b] : (pos_dev ? *pos_dev : pos_arg);
  if (ROWS && (pos < 0 || pos >= Tmax)) return;
  const int C = n_head * DHS;
  const bf16_t* row = qkv + (long long)b * 3 * C + h * DHS;
  float q[DHS], kn[DHS], vn[DHS];
  constexpr int REC = 2 * DHS, CH = DHS / 8;   // record = [k | v] halfs; 16-B chunks per operand
  load_bf16<DHS>(row, q);
  load_bf16<DHS>(row + C, kn);
  load_bf16<DHS>(row + 2 * C, vn);
  bf16_t* seq = cache + ((long long)item * Tmax) * REC;
  if (lane < 2 * CH) {   // append the new record
    const bf16_t* src = (lane < CH) ? row + C + lane * 8 : row + 2 * C + (lane - CH) * 8;
    *reinterpret_cast<uint4*>(seq + (long long)pos * REC + lane * 8) = *reinterpret_cast<const uint4*>(src);
  }
  // scores of this lane's keys (t = lane, lane + 64, ...); the newest key comes from registers, not from the cache
  float m = -INFINITY;
  float sc[4];
  float kv[4][DHS];   // values of this lane's keys
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = lane + 64 * i;
    sc[i] = -INFINITY;
    if (t <= pos) {
      float k[DHS];
      if (t == pos) {
#pragma unroll
        for (int d = 0; d < DHS; ++d) { k[d] = kn[d]; kv[i][d] = vn[d]; }
      } else {
        const bf16_t* sq = ATTN_DECODE_SEQ(t);   // the cached sequence that holds position t of this row
        load_bf16<DHS>(sq + (long long)t * REC, k);
        load_bf16<DHS>(sq + (long long)t * REC + DHS, kv[i]);
      }
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < DHS; ++d) s += q[d] * k[d];
      sc[i] = s * (DHS == 16 ? 0.25f : 0.17677669529663687f);   // 1 / sqrt(hs)
      m = fmaxf(m, sc[i]);
    } else {
#pragma unroll
      for (int d = 0; d < DHS; ++d) kv[i][d] = 0.f;
    }
  }
  m = wave_max(m);
  float l = 0.f, acc[DHS];
#pragma unroll
  for (int d = 0; d < DHS; ++d) acc[d] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float p = (sc[i] == -INFINITY) ? 0.f : __expf(sc[i] - m);
    l += p;
#pragma unroll
    for (int d = 0; d < DHS; ++d) acc[d] += p * kv[i][d];
  }
  l = wave_sum(l);
  const float inv = 1.0f / l;
#pragma unroll
  for (int d = 0; d < DHS; ++d) acc[d] = wave_sum(acc[d]) * inv;
  if (lane == 0) {
    bf16_t* dst = y + (long long)b * C + h * DHS;
#pragma unroll
    for (int i = 0; i < DHS / 8; ++i) *reinterpret_cast<uint4*>(dst + 8 * i) = pack8(acc + 8 * i);
  }
