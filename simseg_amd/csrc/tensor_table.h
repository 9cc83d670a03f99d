// The tensor-table contract of the table-driven passes (optim.hip: AdamW, its gradient checks and LARS; the host side is
// simseg_amd.optim.TensorTable).  One launch serves every tensor of a bucket:
//   table[t]      six 8-byte words per tensor.  Word 0 = the fp32 master, word 1 = its fp32 gradient; the other four belong to the pass
//                 (AdamTensors, LarsTensors: each static_asserts its 48 bytes).
//   sizes[t]      elements of tensor t.
//   chunk_tid[c], chunk_off[c]   chunk c covers elements [chunk_off[c], min(sizes[t], chunk_off[c] + chunk)) of tensor t = chunk_tid[c].
// The grid is one block per chunk; a tensor without elements has no chunk.
#pragma once

// What a block works on: tensor t, its row T and the element range [lo, hi) of the block's chunk.  The row is read between the index and
// the range and the result filled in place: the order and the form in which every kernel did this itself, so that their code stays what
// it was.  A kernel that uses a single field of the row loads that field only.
template <typename Row> struct TableChunk { int t; Row T; long lo, hi; };

template <typename Row>
__device__ __forceinline__ TableChunk<Row> table_chunk(const Row* __restrict__ table, const long* __restrict__ sizes,
                                                       const int* __restrict__ chunk_tid, const long* __restrict__ chunk_off, int chunk) {
    const int c = blockIdx.x;
    TableChunk<Row> r;
    r.t = chunk_tid[c];
    r.T = table[r.t];
    r.lo = chunk_off[c];
    r.hi = min(sizes[r.t], r.lo + chunk);
    return r;
}
