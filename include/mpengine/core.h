/*
 * mpengine/core.h - status codes, enums, mpStream_t and the runtime entry points.
 * Defined in csrc/: mp_runtime.hip.
 * Part of the C ABI of libmpengine.so: the conventions are stated in mpengine.h, the umbrella.
 */
#ifndef MPENGINE_CORE_H
#define MPENGINE_CORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mpStream_t; /* hipStream_t */

enum mp_status { MP_OK = 0, MP_EINVAL = -1, MP_EINDEX = -2, MP_EHIP = -3, MP_ENOTSUP = -4 };

/* kgcnn/ops/segment.py:39-46 names -> op */
enum mp_reduce_op { MP_SUM = 0, MP_MEAN = 1, MP_MAX = 2, MP_MIN = 3 };

/* Activations reachable from SchNet / PaiNN / GCN configs (kgcnn/ops/activ.py:6-15, Keras strings) */
enum mp_activation {
  MP_ACT_LINEAR = 0, MP_ACT_RELU = 1, MP_ACT_SHIFTED_SOFTPLUS = 2, MP_ACT_SOFTPLUS = 3, MP_ACT_SWISH = 4,
  MP_ACT_SIGMOID = 5, MP_ACT_TANH = 6, MP_ACT_LEAKY_RELU = 7,
  MP_ACT_SOFTPLUS2 = 8, /* kgcnn/ops/activ.py:19-29: relu(x) + log(0.5 exp(-|x|) + 0.5) */
  MP_ACT_SELU = 9,      /* Keras "selu" (kgcnn/literature/NMPN.py:41): scale * (x > 0 ? x : alpha * (exp(x) - 1)) */
  MP_ACT_ELU = 10,      /* Keras "elu", alpha = 1 (kgcnn/layers/conv/attentivefp_conv.py:38): x > 0 ? x : exp(x) - 1 */
  MP_ACT_LAST = MP_ACT_ELU
};

enum mp_binary_op { MP_ADD = 0, MP_SUB = 1, MP_MUL = 2 };

/* bits of the device flag word written by mp_index_prepare_i64 */
enum mp_index_flag { MP_FLAG_OOB = 1, MP_FLAG_UNSORTED_COL0 = 2, MP_FLAG_UNSORTED_COL1 = 4 };
/* bit of the flag word of mp_scaler_apply: an atomic number inside [0, 95) that the fit did not see */
enum mp_scaler_flag { MP_FLAG_UNKNOWN_SPECIES = 8 };

/* element types of the host packer (mp_pack_*_host) */
enum mp_dtype { MP_DT_F32 = 0, MP_DT_F64 = 1, MP_DT_I32 = 2, MP_DT_I64 = 3 };

/* ---------------------------------------------------------------- runtime -------------------------------- */
const char* mp_last_error(void);
int mp_version(void);
/* Fills name (<= name_len bytes), CU count and LDS bytes per CU of the current HIP device. */
int mp_device_info(char* name_host, int name_len, int* num_cu_host, int* lds_bytes_host);

/* HIP-graph capture of a launch sequence on `stream` (replaces eager per-op dispatch of Keras/TF). */
int mp_graph_begin(mpStream_t stream);
int mp_graph_end(mpStream_t stream, void** graph_exec_out_host);
int mp_graph_launch(void* graph_exec, mpStream_t stream);
int mp_graph_destroy(void* graph_exec);

/* HIP events on the caller's stream, for timing inside bench.py. */
int mp_event_create(void** event_out_host);
int mp_event_record(void* event, mpStream_t stream);
int mp_event_elapsed_ms(void* start, void* stop, float* ms_out_host); /* synchronises on `stop` */
int mp_event_destroy(void* event);

#ifdef __cplusplus
}
#endif
#endif /* MPENGINE_CORE_H */
