/* Stage-level hooks of libc_eth_kzg for the kernel parity tests under tests/ -- NOT part of the drop-in ABI
 * (bindings/c of the reference has nothing like them).  Kept out of c_eth_kzg.h so that consumers never see them. */
#ifndef C_ETH_KZG_TEST_HOOKS_H
#define C_ETH_KZG_TEST_HOOKS_H
#include "c_eth_kzg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* canonical big-endian encodings; return 0 on success */
int eth_kzg_amd_test_fr_ntt4096(const DASContext *ctx, const uint8_t *in, uint8_t *out, int inverse_dit);
int eth_kzg_amd_test_g1_fft128(const DASContext *ctx, const uint8_t *in, uint8_t *out, int n_lanes, int inverse);
int eth_kzg_amd_test_fixed_msm(const DASContext *ctx, const uint8_t *scalars, int n_msm, uint8_t *out);
int eth_kzg_amd_test_g1_decompress(const DASContext *ctx, const uint8_t *in, int n, int subgroup_check, int32_t *status,
                                   uint8_t *out);
int eth_kzg_amd_test_field_mul(const DASContext *ctx, const uint8_t *a, const uint8_t *b, uint8_t *out, int n,
                               int is_fp);

/* One field or point operation of the kernels per element (csrc/k_test_ops.hip), on the raw words of the device structs.
 * eth_kzg_amd_test_op_info: word counts per element of operation `op` (0, 1, ... until it returns -1), whether it exists on the
 * device only (the pair / quad forms, the tree folds) and its name.  eth_kzg_amd_test_op: n elements of in_words each in, n of
 * out_words each out; on_device = 0 runs the host pass of the same source (ctx may be NULL; an error for the device-only forms). */
int eth_kzg_amd_test_op_info(int op, int32_t *in_words, int32_t *out_words, int32_t *device_only, const char **name);
int eth_kzg_amd_test_op(const DASContext *ctx, int op, int n, const int32_t *in, int32_t *out, int on_device);

#ifdef __cplusplus
}
#endif
#endif /* C_ETH_KZG_TEST_HOOKS_H */
