// Native replay of a recorded launch sequence: one call per forward instead of the reference's
// per-layer Python dispatch (models.py:524-545).  Host-only code; compiled with the kernels so the
// shared library is self-contained.
#include <string.h>

#include <new>
#include <vector>

#include "common.h"

namespace {

union AnyDesc {
    yh_conv_desc conv;
    yh_stem_desc stem;
    yh_pool_desc pool;
    yh_copy_desc copy;
    yh_add_desc add;
    yh_decode_desc decode;
    yh_decode_sxy_desc decode_sxy;
    yh_dw_desc dw;
    yh_se_desc se;
    yh_qcopy_desc qcopy;
    yh_qadd_desc qadd;
    yh_bn_desc bn;
    yh_wgrad_desc wgrad;
    yh_resample_desc resample;
    yh_cast_desc cast;
    yh_layout_desc layout;
    yh_pool_bwd_desc pool_bwd;
    yh_pack_batch_desc pack_batch;
    yh_dw_bwd_desc dw_bwd;
    yh_se_bwd_desc se_bwd;
    yh_stem_bwd_desc stem_bwd;
};

struct Fixup {
    int field_offset;
    int slot;
    int64_t byte_offset;
};

struct Op {
    int kind;
    AnyDesc d;
    std::vector<Fixup> fixups;
};

size_t desc_size(int kind) {
    switch (kind) {
        case YH_OP_CONV: return sizeof(yh_conv_desc);
        case YH_OP_STEM: return sizeof(yh_stem_desc);
        case YH_OP_POOL: return sizeof(yh_pool_desc);
        case YH_OP_COPY: return sizeof(yh_copy_desc);
        case YH_OP_ADD: return sizeof(yh_add_desc);
        case YH_OP_DECODE: return sizeof(yh_decode_desc);
        case YH_OP_DECODE_SXY: return sizeof(yh_decode_sxy_desc);
        case YH_OP_DW: return sizeof(yh_dw_desc);
        case YH_OP_SE: return sizeof(yh_se_desc);
        case YH_OP_QCOPY: return sizeof(yh_qcopy_desc);
        case YH_OP_QPOOL: return sizeof(yh_pool_desc);
        case YH_OP_QADD: case YH_OP_QADD_CLAMPED: return sizeof(yh_qadd_desc);
        case YH_OP_BN_STATS: case YH_OP_BN_FINALIZE: case YH_OP_BN_ACT_FWD: case YH_OP_BN_BWD_REDUCE: case YH_OP_BN_BWD_APPLY:
            return sizeof(yh_bn_desc);
        case YH_OP_WGRAD: case YH_OP_STEM_WGRAD: return sizeof(yh_wgrad_desc);
        case YH_OP_DILATE2: case YH_OP_UPSAMPLE2_BWD: return sizeof(yh_resample_desc);
        case YH_OP_CAST_F32: return sizeof(yh_cast_desc);
        case YH_OP_NCHW_TO_NHWC: return sizeof(yh_layout_desc);
        case YH_OP_POOL_BWD: return sizeof(yh_pool_bwd_desc);
        case YH_OP_PACK_BATCH: return sizeof(yh_pack_batch_desc);
        case YH_OP_DW_WGRAD: case YH_OP_DW_DGRAD: return sizeof(yh_dw_bwd_desc);
        case YH_OP_SE_BWD: return sizeof(yh_se_bwd_desc);
        case YH_OP_STEM_BWD: return sizeof(yh_stem_bwd_desc);
        default: return 0;
    }
}

int launch(int kind, const AnyDesc& d, void* stream) {
    switch (kind) {
        case YH_OP_CONV: return yh_conv2d_fwd(&d.conv, stream);
        case YH_OP_STEM: return yh_conv2d_stem_fwd(&d.stem, stream);
        case YH_OP_POOL: return yh_maxpool2d_fwd(&d.pool, stream);
        case YH_OP_COPY: return yh_copy_channels(&d.copy, stream);
        case YH_OP_ADD: return yh_add_channels(&d.add, stream);
        case YH_OP_DECODE: return yh_yolo_decode(&d.decode, stream);
        case YH_OP_DECODE_SXY: return yh_yolo_decode_sxy(&d.decode_sxy, stream);
        case YH_OP_DW: return yh_dwconv2d_fwd(&d.dw, stream);
        case YH_OP_SE: return yh_se_fwd(&d.se, stream);
        case YH_OP_QCOPY: return yh_qcopy(&d.qcopy, stream);
        case YH_OP_QPOOL: return yh_qpool(&d.pool, stream);
        case YH_OP_QADD: return yh_qadd(&d.qadd, stream);
        case YH_OP_QADD_CLAMPED: return yh_qadd_clamped(&d.qadd, stream);
        case YH_OP_BN_STATS: return yh_bn_stats(&d.bn, stream);
        case YH_OP_BN_FINALIZE: return yh_bn_finalize(&d.bn, stream);
        case YH_OP_BN_ACT_FWD: return yh_bn_act_fwd(&d.bn, stream);
        case YH_OP_BN_BWD_REDUCE: return yh_bn_act_bwd_reduce(&d.bn, stream);
        case YH_OP_BN_BWD_APPLY: return yh_bn_act_bwd_apply(&d.bn, stream);
        case YH_OP_WGRAD: return yh_conv2d_wgrad(&d.wgrad, stream);
        case YH_OP_STEM_WGRAD: return yh_stem_wgrad(&d.wgrad, stream);
        case YH_OP_DILATE2: return yh_dilate2(&d.resample, stream);
        case YH_OP_UPSAMPLE2_BWD: return yh_upsample2_bwd(&d.resample, stream);
        case YH_OP_CAST_F32: return yh_cast_f32(&d.cast, stream);
        case YH_OP_POOL_BWD: return yh_maxpool2d_bwd(&d.pool_bwd, stream);
        case YH_OP_PACK_BATCH: return yh_pack_batch(d.pack_batch.items, d.pack_batch.n_items, stream);
        case YH_OP_DW_WGRAD: return yh_dw_wgrad(&d.dw_bwd, stream);
        case YH_OP_DW_DGRAD: return yh_dw_dgrad(&d.dw_bwd, stream);
        case YH_OP_SE_BWD: return yh_se_bwd(&d.se_bwd, stream);
        case YH_OP_STEM_BWD: return yh_stem_bwd(&d.stem_bwd, stream);
        case YH_OP_NCHW_TO_NHWC:
            return yh_nchw_to_nhwc(d.layout.x, d.layout.y, d.layout.n, d.layout.c, d.layout.h, d.layout.w_in, d.layout.c_pad,
                                   d.layout.ldy, d.layout.dtype, stream);
        default: return YH_EINVAL;
    }
}

}  // namespace

struct yh_plan {
    std::vector<Op> ops;
    std::vector<void*> slots;
    // optional per-op HIP-event timing (bench.py roofline leg): events[2*i], events[2*i+1] bracket op i
    bool timing = false;
    std::vector<hipEvent_t> events;
    // optional hipGraph of one replay (launch-bound small batches): valid for the slot pointers bound at capture
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    void drop_graph() {
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        if (graph) (void)hipGraphDestroy(graph);
        graph_exec = nullptr;
        graph = nullptr;
    }
    ~yh_plan() {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        drop_graph();
    }
};

extern "C" int yh_abi_version(void) { return YH_ABI_VERSION; }

extern "C" const char* yh_error_string(int code) {
    switch (code) {
        case YH_OK: return "ok";
        case YH_EINVAL: return "invalid argument";
        case YH_EALIGN: return "misaligned pointer, pitch or channel count";
        case YH_EUNSUPPORTED: return "unsupported configuration";
        case YH_ENOMEM: return "out of host memory";
        case YH_ERANGE: return "index out of range";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

extern "C" yh_plan* yh_plan_create(void) { return new (std::nothrow) yh_plan(); }

extern "C" void yh_plan_destroy(yh_plan* p) { delete p; }

extern "C" int yh_plan_add(yh_plan* p, int op_kind, const void* desc, int desc_bytes) {
    if (!p || !desc) return YH_EINVAL;
    const size_t want = desc_size(op_kind);
    if (want == 0 || (size_t)desc_bytes != want) return YH_EINVAL;
    Op op;
    op.kind = op_kind;
    memset(&op.d, 0, sizeof(op.d));
    memcpy(&op.d, desc, want);
    try {
        p->ops.push_back(op);
    } catch (...) {
        return YH_ENOMEM;
    }
    return (int)p->ops.size() - 1;
}

extern "C" int yh_plan_add_fixup(yh_plan* p, int op_index, int field_offset, int slot, int64_t byte_offset) {
    if (!p) return YH_EINVAL;
    if (op_index < 0 || op_index >= (int)p->ops.size() || slot < 0 || slot >= 64) return YH_ERANGE;
    Op& op = p->ops[op_index];
    if (field_offset < 0 || (size_t)field_offset + sizeof(void*) > desc_size(op.kind) || field_offset % (int)sizeof(void*)) return YH_ERANGE;
    try {
        op.fixups.push_back(Fixup{field_offset, slot, byte_offset});
        if ((int)p->slots.size() <= slot) p->slots.resize(slot + 1, nullptr);
    } catch (...) {
        return YH_ENOMEM;
    }
    return YH_OK;
}

extern "C" int yh_plan_bind_slot(yh_plan* p, int slot, void* ptr) {
    if (!p) return YH_EINVAL;
    if (slot < 0 || slot >= 64) return YH_ERANGE;
    try {
        if ((int)p->slots.size() <= slot) p->slots.resize(slot + 1, nullptr);
    } catch (...) {
        return YH_ENOMEM;
    }
    p->slots[slot] = ptr;
    return YH_OK;
}

extern "C" int yh_plan_num_ops(const yh_plan* p) { return p ? (int)p->ops.size() : YH_EINVAL; }

// Scheduling hints of ABI 2, accepted and ignored: every op runs in index order on the caller's stream, which satisfies any dependency
// that can be declared (dep < op).  The argument checks and their return codes are the ones the entries always had.
extern "C" int yh_plan_set_lane(yh_plan* p, int op_index, int lane) {
    if (!p) return YH_EINVAL;
    if (op_index < 0 || op_index >= (int)p->ops.size() || lane < 0 || lane > 1) return YH_ERANGE;
    return YH_OK;
}

extern "C" int yh_plan_add_dep(yh_plan* p, int op_index, int dep_index) {
    if (!p) return YH_EINVAL;
    if (op_index < 0 || op_index >= (int)p->ops.size() || dep_index < 0 || dep_index >= op_index) return YH_ERANGE;
    return YH_OK;
}

extern "C" int yh_plan_set_async_reduce(yh_plan* p, int enable) {
    (void)enable;
    return p ? YH_OK : YH_EINVAL;
}

extern "C" int yh_plan_run_range(yh_plan* p, int first, int last, void* stream) {
    if (!p) return YH_EINVAL;
    if (first < 0 || last > (int)p->ops.size() || first > last) return YH_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    for (int i = first; i < last; ++i) {
        const Op& op = p->ops[i];
        AnyDesc d = op.d;
        for (const Fixup& f : op.fixups) {
            void* base = p->slots[f.slot];
            if (!base) return YH_EINVAL;                                   // never bound: a bug in the caller
            void* v = base == YH_SLOT_NULL ? nullptr : (void*)((char*)base + f.byte_offset);   // bound to "nothing": optional outputs
            memcpy((char*)&d + f.field_offset, &v, sizeof(void*));
        }
        if (p->timing) (void)hipEventRecord(p->events[2 * i], s);
        const int rc = launch(op.kind, d, s);
        if (p->timing) (void)hipEventRecord(p->events[2 * i + 1], s);
        if (rc != YH_OK) return rc;
    }
    return YH_OK;
}

extern "C" int yh_plan_set_timing(yh_plan* p, int enable) {
    if (!p) return YH_EINVAL;
    if (enable && p->events.size() < 2 * p->ops.size()) {
        try {
            p->events.reserve(2 * p->ops.size());
        } catch (...) {
            return YH_ENOMEM;
        }
        while (p->events.size() < 2 * p->ops.size()) {
            hipEvent_t e;
            const hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return (int)rc;
            p->events.push_back(e);
        }
    }
    p->timing = enable != 0;
    return YH_OK;
}

extern "C" int yh_plan_get_timings(yh_plan* p, float* ms_out, int n) {
    if (!p || !ms_out) return YH_EINVAL;
    if (n != (int)p->ops.size() || p->events.size() < 2 * p->ops.size()) return YH_ERANGE;
    for (int i = 0; i < n; ++i) {
        const hipError_t rc = hipEventElapsedTime(&ms_out[i], p->events[2 * i], p->events[2 * i + 1]);
        if (rc != hipSuccess) return (int)rc;
    }
    return YH_OK;
}

extern "C" int yh_plan_run(yh_plan* p, void* stream) {
    if (!p) return YH_EINVAL;
    return yh_plan_run_range(p, 0, (int)p->ops.size(), stream);
}


// ---- hipGraph replay -----------------------------------------------------------------------------------
// Captures one replay of the plan (with the currently bound slot pointers) on `stream` into an executable
// graph; yh_plan_graph_launch then costs one graph launch instead of ~100 kernel launches.  The caller keeps
// the slot buffers static between capture and launches (engine/plan.py stages the frame into a fixed buffer).
extern "C" int yh_plan_graph_capture(yh_plan* p, void* stream) {
    if (!p || !stream) return YH_EINVAL;  // capture needs a real (non-null) stream
    p->drop_graph();
    const bool was_timing = p->timing;
    p->timing = false;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) { p->timing = was_timing; return (int)e; }
    const int rc = yh_plan_run_range(p, 0, (int)p->ops.size(), stream);
    e = hipStreamEndCapture(s, &p->graph);
    p->timing = was_timing;
    if (rc != YH_OK) { p->drop_graph(); return rc; }
    if (e != hipSuccess) { p->drop_graph(); return (int)e; }
    e = hipGraphInstantiate(&p->graph_exec, p->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { p->drop_graph(); return (int)e; }
    return YH_OK;
}

extern "C" int yh_plan_graph_launch(yh_plan* p, void* stream) {
    if (!p || !p->graph_exec) return YH_EINVAL;
    const hipError_t e = hipGraphLaunch(p->graph_exec, (hipStream_t)stream);
    return e == hipSuccess ? YH_OK : (int)e;
}

extern "C" int yh_plan_graph_reset(yh_plan* p) {
    if (!p) return YH_EINVAL;
    p->drop_graph();
    return YH_OK;
}
