// SHA-256 of MANY independent messages: the Fiat-Shamir challenges of a batch of EIP-4844 blob proofs
// (compute_fiat_shamir_challenge, crates/eip4844/src/verifier.rs:155-196) without the blobs leaving the GPU.
//
// One lane per message.  SHA-256 is serial inside a message (every 64-byte block needs the state the block before it left),
// so the parallelism is across messages: message i = prefix | body + i * body_stride | tail + i * tail_stride, the three
// lengths uniform per launch; the standard padding (0x80, zeroes, the bit length as 64 big-endian bits) is applied here and the
// digest goes to out + 32 i.  The product's shape: prefix = the 32-byte header "FSBLOBVERIFY_V1_" | 4096, body = the blob
// (131072 B, one per 131072-B row of the caller's array), tail = the commitment (48 B): 2050 blocks per message.
//
// Launch shape (DESIGN section 8's rule for lane-per-item kernels): blocks of ONE whole wave, so that the waves of a batch spread
// over the compute units; the lanes behind the last message repeat the last message's work and store nothing -- a wave with a
// handful of active lanes costs what a full one costs, and without divergence at the tail there is nothing to reason about.
//
// Load shape.  Lane l walks its own row, so one load instruction of the wave touches 64 DIFFERENT rows, 128 KiB apart: nothing
// coalesces across lanes, and what decides the traffic is how much of each fetched line a lane uses before the line is evicted.
// A block of the message is 64 bytes = four 16-byte loads (global_load_dwordx4, the widest per-lane access) to one or two
// adjacent 128-byte lines (in the product's shape the 32-byte prefix puts every block at offset 32 mod 64 of its row); they are
// issued together, one block AHEAD of the compression that consumes them: the raw words of block k + 1 sit in 16 registers while
// the 64 rounds of block k run (~1.7 k integer instructions, 4 cycles each on a wave64, against ~900 cycles of an HBM miss), and
// the byte swap to big-endian words happens after the compression, so the wait for the loads is behind the work that hides them.
// The rest of a fetched line belongs to the next block or two and is read within two compressions (a wave keeps 64 lines = 8 KiB
// live, the L2 holds that for every wave of the chip).  With dword loads the same bytes would take sixteen instructions per block
// that each visit 64 lines; with byte loads 64.  The wide path needs the
// block to lie wholly inside the body at a 16-byte-aligned address (every block of a blob but the first and the last two, for
// buffers from hipMalloc / torch): blocks that straddle prefix | body | tail, the padding, and bodies at odd addresses are
// gathered byte by byte -- correct for every split of the lengths, and three blocks of 2050 in the product's shape.
//
// Plain C++: rotates as the compiler lowers them (v_alignbit_b32), no inline assembly, ordinary vector stores; one scheduling
// builtin keeps the prefetch in front of the rounds (checked in the ISA: wait, swap, four loads, then the 64 rounds).
//
// Second kernel, behind the first: k_sha256_cell_leaves, the per-cell leaves of the cell verifier's leaf-hashed challenge.
#include "launch.hpp"

#include <stdexcept>

namespace kzg {
namespace {

__constant__ const uint32_t SHA256_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// one block: w = its sixteen big-endian words (overwritten by the message schedule)
__device__ __forceinline__ void sha256_compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            const uint32_t w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
            w[t & 15] += (rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3)) + w[(t - 7) & 15] + (rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + SHA256_K[t] + w[t & 15];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

struct Message {
    const uint8_t *prefix, *body, *tail;  // body / tail: this lane's
    uint64_t prefix_len, body_end, total;  // body_end = prefix_len + body_len, total = body_end + tail_len
};
// the padded message's byte at position p (p below the padded length; the bit length is patched in by the caller)
__device__ __forceinline__ uint32_t padded_byte(const Message& m, uint64_t p) {
    if (p < m.prefix_len) return m.prefix[p];
    if (p < m.body_end) return m.body[p - m.prefix_len];
    if (p < m.total) return m.tail[p - m.body_end];
    return p == m.total ? 0x80u : 0u;
}
// the block at `off` of the padded message, gathered byte by byte, as big-endian words
__device__ __forceinline__ void gather_block(const Message& m, uint64_t off, bool last, uint32_t (&w)[16]) {
#pragma unroll 1
    for (int j = 0; j < 16; j++) {
        uint32_t v = 0;
        for (int k = 0; k < 4; k++) v = (v << 8) | padded_byte(m, off + 4 * j + k);
        w[j] = v;
    }
    if (last) {  // the message length in bits, 64 bits big-endian, in the block's last eight bytes
        const uint64_t bits = m.total * 8;
        w[14] = (uint32_t)(bits >> 32);
        w[15] = (uint32_t)bits;
    }
}
// 64 aligned bytes as four 16-byte loads; the words as the little-endian loads deliver them
__device__ __forceinline__ void load_block_wide(const uint8_t* p, uint32_t (&raw)[16]) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint4 v = q[j];
        raw[4 * j] = v.x; raw[4 * j + 1] = v.y; raw[4 * j + 2] = v.z; raw[4 * j + 3] = v.w;
    }
}

__global__ __launch_bounds__(64) void k_sha256_many(int n, const uint8_t* __restrict__ prefix, uint32_t prefix_len,
                                                    const uint8_t* __restrict__ body, size_t body_stride, uint32_t body_len,
                                                    const uint8_t* __restrict__ tail, size_t tail_stride, uint32_t tail_len,
                                                    uint8_t* __restrict__ out) {
    const int lane_msg = blockIdx.x * 64 + threadIdx.x;
    const int i = lane_msg < n ? lane_msg : n - 1;
    Message m;
    m.prefix = prefix;
    m.body = body + (size_t)i * body_stride;
    m.tail = tail + (size_t)i * tail_stride;
    m.prefix_len = prefix_len;
    m.body_end = m.prefix_len + body_len;
    m.total = m.body_end + tail_len;
    const uint64_t n_blocks = (m.total + 9 + 63) / 64;  // 0x80 and the eight length bytes always fit
    // blocks [wide0, wide1) lie wholly inside the body; they take the wide loads if this lane's row puts them at 16-byte-aligned
    // addresses (blocks are 64 bytes apart: one test decides for all of them)
    const uint64_t wide0 = (m.prefix_len + 63) / 64;
    uint64_t wide1 = m.body_end / 64;
    const uint8_t* wide_base = m.body + wide0 * 64 - m.prefix_len;  // (only dereferenced when the range is not empty)
    if (wide1 < wide0 || (reinterpret_cast<uintptr_t>(wide_base) & 15) != 0) wide1 = wide0;
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint32_t w[16];
    // two passes of the gathered form around the wide loop: the blocks in front of the wide range, then those behind it
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        const uint64_t k0 = pass ? wide1 : 0, k1 = pass ? n_blocks : wide0;
#pragma unroll 1
        for (uint64_t k = k0; k < k1; k++) {
            gather_block(m, k * 64, k + 1 == n_blocks, w);
            sha256_compress(h, w);
        }
        if (pass == 0 && wide0 < wide1) {
            uint32_t raw[16];
            load_block_wide(wide_base, raw);
#pragma unroll 1
            for (uint64_t k = wide0; k < wide1; k++) {
#pragma unroll
                for (int j = 0; j < 16; j++) w[j] = __builtin_bswap32(raw[j]);
                // the next block's loads are in flight under the 64 rounds below (the last iteration reloads its own block: no branch)
                load_block_wide(wide_base + (size_t)((k + 1 < wide1 ? k + 1 : k) - wide0) * 64, raw);
                __builtin_amdgcn_sched_barrier(0);  // the scheduler would sink the loads behind the rounds (fewer live registers) and then wait for them
                sha256_compress(h, w);
            }
        }
    }
    if (lane_msg >= n) return;
    uint8_t* o = out + (size_t)i * 32;
    if ((reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        uint4* q = reinterpret_cast<uint4*>(o);
        q[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
        q[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]), __builtin_bswap32(h[7]));
    } else {
        for (int j = 0; j < 32; j++) o[j] = (uint8_t)(h[j >> 2] >> (24 - 8 * (j & 3)));
    }
}

// ---- The leaves of the cell verifier's leaf-hashed challenge (verify_host.hpp: CellLeafTranscript), straight out of the verifier's
// arena as stage_and_decode (verify.hip) leaves it:
//   leaf k = SHA-256("RCKZGCBATCHLEAF1" | be64(k) | be64(idx[k]) | uniq[row[k]] (48 B) | proofs[k] (48 B) | cells[k] (2048 B))
// 2176 bytes = 34 blocks of the message and a 35th of constant padding.  One lane per cell, blocks of one whole wave, the lanes
// behind the last cell repeat its work and store nothing: the launch shape of k_sha256_many and its reasons.
// The uniform layout takes the place of k_sha256_many's general gather: the header is exactly two blocks, built in registers
// from the position, the index and six 16-byte loads (a commitment and a proof are 48 bytes at 48-byte strides from 256-byte-
// aligned offsets of the arena); every 64-byte row of the cell is one block and takes the wide loads, one block ahead of the
// compression, as above -- lane l walks its own 2 KiB row, so the argument of this file's header about lines and latency holds
// with rows 2 KiB apart instead of 128 KiB; the padding block is three constants.  A batch of 8192 cells is 128 waves on a chip
// with 1024 SIMDs: while every wave has a SIMD to itself the launch lasts what ONE lane's 35 dependent compressions last
// (about 0.2 ms with the read-back and the root), and it leaves the chip to the decoding kernels next to it.
// The launcher refuses pointers that do not have the alignments the wide loads and stores assume.
// Two instantiations.  POSITIONS = false is the single verification's kernel: the hashed position of cell i is i.  POSITIONS = true is
// the many-verification's (verify_many.hip): its arena holds the cells of all the problems of a pass back to back, uniq / row / idx /
// proofs / cells are pass-wide, and the hashed position is pos[i], the cell's place INSIDE its problem (it restarts at 0 in each one).
constexpr uint32_t be32_of(const char* s) {
    return ((uint32_t)(uint8_t)s[0] << 24) | ((uint32_t)(uint8_t)s[1] << 16) | ((uint32_t)(uint8_t)s[2] << 8) | (uint32_t)(uint8_t)s[3];
}
// "RCKZGCBATCHLEAF1" as four big-endian words
constexpr uint32_t LEAF_DOMAIN_0 = be32_of("RCKZ"), LEAF_DOMAIN_1 = be32_of("GCBA"), LEAF_DOMAIN_2 = be32_of("TCHL"), LEAF_DOMAIN_3 = be32_of("EAF1");
constexpr uint32_t LEAF_MESSAGE_BITS = (16 + 8 + 8 + 48 + 48 + 2048) * 8;
static_assert(LEAF_MESSAGE_BITS == 17408 && LEAF_MESSAGE_BITS % 512 == 0, "34 whole blocks: the padding is a block of its own");

// 16 aligned bytes as four big-endian words
__device__ __forceinline__ void load16_be(const uint8_t* p, uint32_t* w) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = __builtin_bswap32(v.x); w[1] = __builtin_bswap32(v.y); w[2] = __builtin_bswap32(v.z); w[3] = __builtin_bswap32(v.w);
}
// the blocks that are not rows of the cell: 0 and 1 = the header, 2 = the padding
__device__ __forceinline__ void leaf_edge_block(int which, uint32_t k, uint32_t index, const uint8_t* commitment, const uint8_t* proof,
                                                uint32_t (&w)[16]) {
    if (which == 0) {
        w[0] = LEAF_DOMAIN_0; w[1] = LEAF_DOMAIN_1; w[2] = LEAF_DOMAIN_2; w[3] = LEAF_DOMAIN_3;
        w[4] = 0; w[5] = k;      // be64(k): positions are 32-bit on the device (engine.hpp: MAX_CELLS_PER_VERIFICATION)
        w[6] = 0; w[7] = index;  // be64(index)
        load16_be(commitment, w + 8);
        load16_be(commitment + 16, w + 12);
    } else if (which == 1) {
        load16_be(commitment + 32, w);
        load16_be(proof, w + 4);
        load16_be(proof + 16, w + 8);
        load16_be(proof + 32, w + 12);
    } else {
        w[0] = 0x80000000u;
#pragma unroll
        for (int j = 1; j < 15; j++) w[j] = 0;
        w[15] = LEAF_MESSAGE_BITS;
    }
}

template <bool POSITIONS>
__global__ __launch_bounds__(64) void k_sha256_cell_leaves(int n, const uint8_t* __restrict__ uniq, const int* __restrict__ row,
                                                           const int* __restrict__ idx, const int* __restrict__ pos,
                                                           const uint8_t* __restrict__ proofs, const uint8_t* __restrict__ cells,
                                                           uint8_t* __restrict__ out) {
    const int lane_cell = blockIdx.x * 64 + threadIdx.x;
    const int i = lane_cell < n ? lane_cell : n - 1;
    const uint8_t* commitment = uniq + (size_t)row[i] * 48;
    const uint8_t* proof = proofs + (size_t)i * 48;
    const uint8_t* cell = cells + (size_t)i * 2048;
    const uint32_t index = (uint32_t)idx[i];
    const uint32_t position = POSITIONS ? (uint32_t)pos[i] : (uint32_t)i;
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint32_t w[16];
    // two passes of the edge blocks around the wide loop (one inlined copy of the rounds each): the header, then the padding
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
#pragma unroll 1
        for (int e = pass ? 2 : 0; e < (pass ? 3 : 2); e++) {
            leaf_edge_block(e, position, index, commitment, proof, w);
            sha256_compress(h, w);
        }
        if (pass == 0) {
            uint32_t raw[16];
            load_block_wide(cell, raw);
#pragma unroll 1
            for (int k = 0; k < 32; k++) {
#pragma unroll
                for (int j = 0; j < 16; j++) w[j] = __builtin_bswap32(raw[j]);
                // the next row's loads are in flight under the 64 rounds below (the last iteration reloads its own row: no branch)
                load_block_wide(cell + (size_t)(k + 1 < 32 ? k + 1 : k) * 64, raw);
                __builtin_amdgcn_sched_barrier(0);  // (as in k_sha256_many: the loads stay in front of the rounds)
                sha256_compress(h, w);
            }
        }
    }
    if (lane_cell >= n) return;
    uint4* q = reinterpret_cast<uint4*>(out + (size_t)i * 32);
    q[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
    q[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]), __builtin_bswap32(h[7]));
}

}  // namespace

namespace launch {
// (launch.hpp: preload_code_objects) this translation unit's code object is loaded with the others, not by a caller's first batch
void preload_k_sha256() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_sha256_many));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_sha256_cell_leaves<false>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_sha256_cell_leaves<true>));
}
void sha256_cell_leaves(int n, const uint8_t* uniq, const int* row, const int* idx, const uint8_t* proofs, const uint8_t* cells, uint8_t* out,
                        hipStream_t st, const int* pos) {
    if (n <= 0) return;
    const uintptr_t loads = reinterpret_cast<uintptr_t>(uniq) | reinterpret_cast<uintptr_t>(proofs) | reinterpret_cast<uintptr_t>(cells);
    const uintptr_t ints = reinterpret_cast<uintptr_t>(row) | reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(pos);
    if ((loads & 15) != 0 || (reinterpret_cast<uintptr_t>(out) & 31) != 0 || (ints & 3) != 0)
        throw std::invalid_argument("sha256_cell_leaves: commitments, proofs and cells must be 16-byte aligned, the digests 32-byte aligned");
    if (pos) k_sha256_cell_leaves<true><<<(n + 63) / 64, 64, 0, st>>>(n, uniq, row, idx, pos, proofs, cells, out);
    else k_sha256_cell_leaves<false><<<(n + 63) / 64, 64, 0, st>>>(n, uniq, row, idx, nullptr, proofs, cells, out);
}
void sha256_many(int n, const uint8_t* prefix, uint32_t prefix_len, const uint8_t* body, size_t body_stride, uint32_t body_len,
                 const uint8_t* tail, size_t tail_stride, uint32_t tail_len, uint8_t* out, hipStream_t st) {
    if (n <= 0) return;
    k_sha256_many<<<(n + 63) / 64, 64, 0, st>>>(n, prefix, prefix_len, body, body_stride, body_len, tail, tail_stride, tail_len, out);
}
}  // namespace launch
}  // namespace kzg
