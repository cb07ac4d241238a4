/*
 * mpengine.h - C ABI of the MI355X-native message-passing engine (libmpengine.so).
 *
 * Drop-in boundary for the ragged scatter-gather hot path of kgcnn (Tacitus523/gcnn_keras):
 * every entry point replaces a short composition of TensorFlow ops inside one reference function,
 * cited as file:line relative to the reference tree.  The reference has no FFI of its own (it is
 * pure Python on TensorFlow); INTEGRATION.md shows the ctypes binding a maintainer adds to
 * kgcnn/layers/{gather,pooling}.py to route through this library.
 *
 * Conventions
 *  - All pointers are DEVICE pointers (HIP, gfx950) unless the name ends in _host.  Plain pointers and
 *    sizes only; no framework types.  Values are float32 row-major; API indices / row_splits are int64
 *    exactly as the reference's RaggedTensor delivers them (kgcnn/data/utils.py:129-157).
 *  - Index convention: idx[e] = (i, j), column 0 = receiving node i, column 1 = sending node j
 *    (reference README.md:66); indices are per-graph local ("sample" indexing, kgcnn/layers/base.py:42-43).
 *  - Every call is asynchronous on the caller's stream (mpStream_t == hipStream_t), re-entrant, and keeps no
 *    pointer after it returns.  The caller allocates every input, output and workspace buffer.
 *  - Return: MP_OK or a negative status; mp_last_error() gives a thread-local message.  Host code maps
 *    MP_EINVAL -> ValueError/TypeError, MP_EINDEX -> IndexError (TF InvalidArgumentError), MP_EHIP -> RuntimeError.
 *  - Out-of-range indices never fault: they are clamped and recorded in a caller-provided device flag word
 *    (the analogue of ragged_validate / TF-GPU's silent zero fill); the caller decides when to read the flag.
 *
 * This is the umbrella: the declarations live in one header per family under mpengine/, each with its own include
 * guard and the csrc/ files that define its entry points named at its top.  Including this file gives all of them.
 */
#include "mpengine/core.h"
#include "mpengine/index.h"
#include "mpengine/gather.h"
#include "mpengine/segment.h"
#include "mpengine/dense.h"
#include "mpengine/wgrad.h"
#include "mpengine/geometry.h"
#include "mpengine/backward.h"
#include "mpengine/schnet.h"
#include "mpengine/schnet_model.h"
#include "mpengine/painn.h"
#include "mpengine/gcn.h"
#include "mpengine/chain.h"
#include "mpengine/batching.h"
#include "mpengine/recurrent.h"
#include "mpengine/hdnnp.h"
#include "mpengine/dimenet.h"
#include "mpengine/egnn.h"
#include "mpengine/cgcnn.h"
#include "mpengine/gat.h"
#include "mpengine/megnet.h"
#include "mpengine/cmpnn.h"
#include "mpengine/dmpnn.h"
#include "mpengine/rgcn.h"
#include "mpengine/attentivefp.h"
#include "mpengine/scaler.h"
#include "mpengine/megan.h"
#include "mpengine/mat.h"
#include "mpengine/topk.h"
#include "mpengine/hamnet.h"
