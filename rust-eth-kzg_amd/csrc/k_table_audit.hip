// The table audit's kernel and its host pass (libc_eth_kzg_hooks.so only): table_audit.hpp over every entry, one thread per entry.
#include "kcommon.hpp"
#include "table_audit.hpp"

namespace kzg {

__global__ __launch_bounds__(256) void k_table_audit(const void* const* __restrict__ blocks, const G1Affine* __restrict__ bases, int c, int nb,
                                                     unsigned long long n_entries, audit::Out* __restrict__ out) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_entries) return;
    audit::audit_entry(blocks, bases, c, nb, e, out);
}

namespace launch {
// out: a device audit::Out whose findings pointer is a device buffer
void table_audit_device(const void* const* blocks, const void* bases, int c, int n_groups, int nb, void* out, hipStream_t st) {
    const unsigned long long n = (unsigned long long)table_glv_entries(c, n_groups, nb);
    if (n == 0) return;
    k_table_audit<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(blocks, (const G1Affine*)bases, c, nb, n, (audit::Out*)out);
}
void table_audit_host(const void* const* blocks, const void* bases, int c, int n_groups, int nb, unsigned long long* visited,
                      unsigned long long* n_findings, int32_t* findings, int max_findings) {
    audit::Out o;
    o.visited = 0;
    o.n_findings = 0;
    o.max_findings = (unsigned)max_findings;
    o.findings = findings;
    const unsigned long long n = (unsigned long long)table_glv_entries(c, n_groups, nb);
    for (unsigned long long e = 0; e < n; e++) audit::audit_entry(blocks, (const G1Affine*)bases, c, nb, e, &o);
    *visited = o.visited;
    *n_findings = o.n_findings;
}
}  // namespace launch
}  // namespace kzg
