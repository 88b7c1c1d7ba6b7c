"""numpy reference of the projection arithmetic of ps_project_* / predictive.Projection: per output the sum
over the input fields in ascending order, starting from +0.0, product and sum rounded separately in float64,
zero weights skipped.  Shared by the CPU and GPU projection tests ("the reference")."""
import numpy as np


def project(fields, W):
    """fields: [nin, *shape] float64, W: [nout, nin] -> [nout, *shape] float64"""
    fields = np.asarray(fields, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    assert W.ndim == 2 and W.shape[1] == fields.shape[0]
    out = np.zeros((W.shape[0],) + fields.shape[1:], dtype=np.float64)
    for e in range(W.shape[0]):
        acc = np.zeros(fields.shape[1:], dtype=np.float64)
        for d in range(W.shape[1]):
            if W[e, d] == 0.0:
                continue
            acc = acc + W[e, d] * fields[d]
        out[e] = acc
    return out
