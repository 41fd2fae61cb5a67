"""Helpers of tests/test_gpu_sidecar_columns.py and tests/test_sidecar_columns_host.py: eth_kzg_amd_blobs_to_data_columns / _device.

Nothing here computes an expected value with the new call: cells come from the oracle, the vectors or the calls the issue names, and
the expected matrices are plain transpositions of them."""
import numpy as np

N_CELLS, CELL_BYTES, PROOF_BYTES, BLOB_BYTES = 128, 2048, 48, 131072
GUARD = 0xA5


def transposed(per_blob):
    """per_blob[i][c] -> columns[c][i]"""
    return [[row[c] for row in per_blob] for c in range(N_CELLS)]


def guard(size):
    return bytes([GUARD]) * size


def expected_columns(per_blob, keep, size):
    """columns[c][i] of a host-form call over a guard pattern: per_blob[i][c] where keep[i], the guard elsewhere"""
    g = guard(size)
    return [[per_blob[i][c] if keep[i] else g for i in range(len(per_blob))] for c in range(N_CELLS)]


def column_bytes(columns):
    """columns[c][i] -> the flat [128][n] matrix"""
    return b"".join(x for col in columns for x in col)


def split_matrix(raw, n, size):
    return [[raw[(c * n + i) * size:(c * n + i + 1) * size] for i in range(n)] for c in range(N_CELLS)]


class DeviceCall:
    """the flat arrays of a list of items (blob, commitment or None, [128 proofs]) and the two output matrices in device memory, over
    the guard pattern; commitments, proofs and out_proofs `shift` bytes into their allocations, blobs and out_cells at a multiple of
    four that is no multiple of sixteen when shift is set.  stream: the inputs are written by a kernel queued on that stream."""

    def __init__(self, items, shift=0, stream=None, want_cells=True, want_proofs=True):
        import torch
        self.torch, self.n, self.keep = torch, len(items), []
        n = self.n
        aligned = ((shift + 3) // 4 * 4 + 4) if shift else 0
        ins = [(b"".join(it[0] for it in items), aligned),
               (b"".join(it[1] for it in items) if all(it[1] is not None for it in items) else None, shift),
               (b"".join(p for it in items for p in it[2]), shift)]
        self.inputs = []
        for raw, off in ins:
            if raw is None:
                self.inputs.append(0)
                continue
            a = torch.from_numpy(np.frombuffer(raw or bytes(1), dtype=np.uint8).copy())
            if stream is None:
                d = torch.empty(off + len(a), dtype=torch.uint8, device="cuda")
                d[off:].copy_(a)
            else:
                with torch.cuda.stream(stream):
                    staged = a.pin_memory().to("cuda", non_blocking=True)
                    d = torch.zeros(off + len(a), dtype=torch.uint8, device="cuda")
                    d[off:] = staged ^ 0  # an elementwise kernel, not a copy engine
                self.keep.append(staged)
            self.keep.append(d)
            self.inputs.append(d.data_ptr() + off)
        self.out = []
        for want, size, off in ((want_cells, CELL_BYTES, aligned), (want_proofs, PROOF_BYTES, shift)):
            if not want:
                self.out.append((None, 0, 0, size))
                continue
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):  # (the fill is in front of the call)
                d = torch.full((off + N_CELLS * max(1, n) * size + 64,), GUARD, dtype=torch.uint8, device="cuda")  # 64 guard bytes behind
            self.out.append((d, d.data_ptr() + off, off, size))
        if stream is None:
            torch.cuda.synchronize()

    def call(self, ctx, verify=False, want_status=True, stream=None):
        return ctx.blobs_to_data_columns_device(self.n, self.inputs[0], self.inputs[1], self.inputs[2], self.out[0][1], self.out[1][1], verify=verify,
                                                want_status=want_status, stream=stream)

    def _matrix(self, k):
        d, _, off, size = self.out[k]
        if d is None:
            return None
        raw = d.cpu().numpy().tobytes()
        assert raw[:off] == guard(off) and raw[off + N_CELLS * self.n * size:] == guard(len(raw) - off - N_CELLS * self.n * size), "bytes around the matrix"
        return split_matrix(raw[off:], self.n, size)

    def cells(self):
        return self._matrix(0)

    def proofs(self):
        return self._matrix(1)
