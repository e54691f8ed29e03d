// rt_comm.hip — RCCL behind the C ABI: the library loaded on first use, the gather of a
// multi-device context's stripes (device_gather) and the one-process-per-GPU exchange
// (rt.h rt_comm_*, rt_gather_image).  No build-dependent code: built once for both libraries.
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>

#include "rt_ctx.h"

namespace rt_impl __attribute__((visibility("hidden"))) {

namespace {

// RCCL, loaded on first use (rt_comm_*, multi-device rt_read_image).  Not linked: a
// single-device context never pays for loading it.
struct Rccl {
    bool tried = false, ok = false;
    void* h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;   // optional: an error inside a group aborts
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    // optional: a non-blocking communicator (rt_comm_init), so that no RCCL call can hold the
    // host past the context's deadline (rt_comm_set_timeout)
    decltype(&ncclCommInitRankConfig) CommInitRankConfig = nullptr;
    decltype(&ncclCommGetAsyncError) CommGetAsyncError = nullptr;
};
Rccl& rccl() {
    static Rccl r;
    if (!r.tried) {
        r.tried = true;
        r.h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!r.h) r.h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (r.h) {
#define RT_SYM(F) r.F = reinterpret_cast<decltype(r.F)>(dlsym(r.h, "nccl" #F))
            RT_SYM(GetUniqueId); RT_SYM(CommInitRank); RT_SYM(CommInitAll); RT_SYM(CommDestroy); RT_SYM(Send);
            RT_SYM(Recv); RT_SYM(GroupStart); RT_SYM(GroupEnd); RT_SYM(GetErrorString); RT_SYM(CommAbort);
            RT_SYM(CommInitRankConfig); RT_SYM(CommGetAsyncError);
#undef RT_SYM
            r.ok = r.GetUniqueId && r.CommInitRank && r.CommInitAll && r.CommDestroy && r.Send && r.Recv &&
                   r.GroupStart && r.GroupEnd && r.GetErrorString;
        }
    }
    return r;
}

#define NCCLCHK(ctx, call)                                                                               \
    do {                                                                                                 \
        ncclResult_t e_ = (call);                                                                        \
        if (e_ != ncclSuccess)                                                                           \
            return set_err(ctx, RT_ERR_DEVICE, std::string(#call) + ": " + rccl().GetErrorString(e_));    \
    } while (0)

// Runs the calls between ncclGroupStart and ncclGroupEnd and closes the group whatever they
// return, so a failed Send / Recv / copy does not leave a group open on this thread (later
// RCCL calls would be queued into it).  The body's error wins over GroupEnd's.  On an error the
// context's communicators are then aborted (ncclCommAbort): the group may have
// submitted a Send whose Recv was never queued (or the reverse), and a later stream
// synchronisation would wait on that unmatched peer forever; aborting frees the queued work and
// the next gather needs rt_comm_init (one process per GPU) or a fresh ncclCommInitAll.
void abort_comms(rt_ctx* c);
template <class F>
int group_body(rt_ctx* c, F&& body) {
    const int r = body();
    ncclResult_t e = rccl().GroupEnd();
    if (e == ncclInProgress && c->comm_nonblocking) e = ncclSuccess;   // completed by comm_wait
    if (r || e != ncclSuccess) abort_comms(c);
    if (r) return r;
    if (e != ncclSuccess) return set_err(c, RT_ERR_DEVICE, std::string("ncclGroupEnd: ") + rccl().GetErrorString(e));
    return RT_OK;
}

// Frees the context's communicators and whatever they still have queued: ncclCommAbort, or
// ncclCommDestroy where the library lacks it (a communicator is never just dropped).
void abort_comms(rt_ctx* c) {
    for (Device& d : c->devs) {
        if (!d.comm) continue;
        if (rccl().CommAbort) (void)rccl().CommAbort(d.comm);
        else (void)rccl().CommDestroy(d.comm);
        d.comm = nullptr;
    }
    c->proc_comm = false;
    c->comm_nonblocking = false;
    c->comm_tried = false;   // a multi-device context makes its communicators again on the next gather
}

// Deadlines of the one-process-per-GPU exchange.  A peer that never joins
// (ncclCommInitRank) or never posts its matching Send / Recv would otherwise hold the host
// forever; with a deadline the call returns RT_ERR_TIMEOUT after aborting the communicator,
// which also ends its queued kernels, and the caller falls back or reports.
using Clock = std::chrono::steady_clock;
Clock::time_point comm_deadline(const rt_ctx* c) {
    return c->comm_timeout_ms > 0 ? Clock::now() + std::chrono::milliseconds(c->comm_timeout_ms)
                                  : Clock::time_point::max();
}

int comm_timeout(rt_ctx* c, const std::string& what) {
    abort_comms(c);
    return set_err(c, RT_ERR_TIMEOUT, what + ": no completion within " + std::to_string(c->comm_timeout_ms) +
                                          " ms (the communicator was aborted; rt_comm_init again)");
}

// The state of a non-blocking communicator's last operation: RT_OK once it is no longer
// ncclInProgress, RT_ERR_DEVICE (communicator aborted) on an asynchronous error, RT_ERR_TIMEOUT
// past the deadline.  A blocking communicator has nothing to wait for.
int comm_wait(rt_ctx* c, ncclComm_t comm, Clock::time_point deadline, const char* what) {
    if (!c->comm_nonblocking || !rccl().CommGetAsyncError) return RT_OK;
    for (;;) {
        ncclResult_t st = ncclSuccess;
        const ncclResult_t e = rccl().CommGetAsyncError(comm, &st);
        if (e != ncclSuccess) st = e;
        if (st == ncclSuccess) return RT_OK;
        if (st != ncclInProgress) {
            abort_comms(c);
            return set_err(c, RT_ERR_DEVICE, std::string(what) + ": " + rccl().GetErrorString(st));
        }
        if (Clock::now() >= deadline) return comm_timeout(c, what);
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}

// hipStreamSynchronize with the deadline: polls the stream (and the communicator's asynchronous
// error) instead of blocking in the runtime.
int stream_wait(rt_ctx* c, Device& d, Clock::time_point deadline, const char* what) {
    for (;;) {
        const hipError_t e = hipStreamQuery(d.stream);
        if (e == hipSuccess) return RT_OK;
        if (e != hipErrorNotReady) {
            abort_comms(c);
            return set_err(c, RT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
        }
        if (d.comm && c->comm_nonblocking && rccl().CommGetAsyncError) {
            ncclResult_t st = ncclSuccess;
            if (rccl().CommGetAsyncError(d.comm, &st) == ncclSuccess && st != ncclSuccess && st != ncclInProgress) {
                abort_comms(c);
                return set_err(c, RT_ERR_DEVICE, std::string(what) + ": " + rccl().GetErrorString(st));
            }
        }
        if (Clock::now() >= deadline) return comm_timeout(c, what);
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}

}  // namespace

// Multi-device context: device k's stripe block (local_rows x W, in its padded slot) into
// device 0's gather buffer, then the de-interleave kernel into device 0's full image.
// RCCL (ncclCommInitAll over the context's devices, one ncclSend per device k > 0 and the
// matching ncclRecv on device 0, grouped) when the device ids are distinct and RCCL
// loads; peer copies otherwise (several slots on one device: RCCL allows one rank per
// device).  The renders were synchronised by the caller.
int device_gather(rt_ctx* c) {
    const int ndev = (int)c->devs.size();
    const int padded = padded_rows_of(c->height, ndev, c->stripe_rows);
    const size_t slot = (size_t)padded * c->width * 16;
    Device& d0 = c->devs[0];
    if (ensure(c, d0, d0.gather, slot * ndev) || ensure(c, d0, d0.full, (size_t)c->height * c->width * 16))
        return RT_ERR_DEVICE;
    if (!c->comm_tried) {
        c->comm_tried = true;
        bool distinct = true;
        for (int i = 0; i < ndev; i++)
            for (int j = 0; j < i; j++) distinct = distinct && c->devs[i].id != c->devs[j].id;
        if (distinct && rccl().ok) {
            std::vector<ncclComm_t> comms(ndev, nullptr);
            std::vector<int> ids(ndev);
            for (int k = 0; k < ndev; k++) ids[k] = c->devs[k].id;
            if (rccl().CommInitAll(comms.data(), ndev, ids.data()) == ncclSuccess)
                for (int k = 0; k < ndev; k++) c->devs[k].comm = comms[k];
        }
    }
    if (d0.comm) {
        NCCLCHK(c, rccl().GroupStart());
        // the group is closed on every path: an error inside it is returned after GroupEnd
        int in_group = group_body(c, [&]() -> int {
            for (int k = 0; k < ndev; k++) {
                Device& d = c->devs[k];
                const size_t n = (size_t)d.local_rows * c->width * 4;   // floats of the block
                char* dst = (char*)d0.gather.ptr + slot * k;
                HIPCHK(c, hipSetDevice(d.id));
                if (k == 0) {
                    HIPCHK(c, hipMemcpyAsync(dst, d.image_ptr, n * 4, hipMemcpyDeviceToDevice, d0.stream));
                } else if (n) {
                    NCCLCHK(c, rccl().Send(d.image_ptr, n, ncclFloat, 0, d.comm, d.stream));
                    NCCLCHK(c, rccl().Recv(dst, n, ncclFloat, k, d0.comm, d0.stream));
                }
            }
            return RT_OK;
        });
        if (in_group) return in_group;
        for (Device& d : c->devs) {
            HIPCHK(c, hipSetDevice(d.id));
            HIPCHK(c, hipStreamSynchronize(d.stream));
        }
        c->gather_path = RT_GATHER_RCCL;
    } else {
        HIPCHK(c, hipSetDevice(d0.id));
        for (int k = 0; k < ndev; k++) {
            Device& d = c->devs[k];
            HIPCHK(c, hipMemcpyPeerAsync((char*)d0.gather.ptr + slot * k, d0.id, d.image_ptr, d.id,
                                         (size_t)d.local_rows * c->width * 16, d0.stream));
        }
        c->gather_path = RT_GATHER_PEER;
    }
    HIPCHK(c, hipSetDevice(d0.id));
    if (rt_launch_deinterleave(d0.gather.ptr, d0.full.ptr, c->width, c->height, ndev, c->stripe_rows, padded,
                               d0.stream))
        return set_err(c, RT_ERR_DEVICE, "de-interleave kernel launch failed");
    HIPCHK(c, hipStreamSynchronize(d0.stream));
    return RT_OK;
}

void comm_destroy(Device& d) {
    if (d.comm && rccl().ok) (void)rccl().CommDestroy(d.comm);
}

}  // namespace rt_impl

using namespace rt_impl;

extern "C" {

// ---- one process per GPU: RCCL behind the ABI (rt.h rt_comm_*) ----------------
int rt_comm_unique_id(void* id_out) {
    if (!id_out) return RT_ERR_INVALID_ARG;
    if (!rccl().ok) return RT_ERR_DEVICE;
    ncclUniqueId id;
    if (rccl().GetUniqueId(&id) != ncclSuccess) return RT_ERR_DEVICE;
    static_assert(sizeof(ncclUniqueId) == RT_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    std::memcpy(id_out, &id, sizeof(id));
    return RT_OK;
}

int rt_comm_init(rt_ctx* c, const void* id, int rank, int world) {
    if (!c || !id) return RT_ERR_INVALID_ARG;
    if (c->devs.size() != 1) return set_err(c, RT_ERR_STATE, "rt_comm_init needs a 1-device context");
    if (world != c->proc_world || rank != c->proc_rank)
        return set_err(c, RT_ERR_STATE, "rt_comm_init: rank / world differ from rt_set_partition's");
    if (!rccl().ok) return set_err(c, RT_ERR_DEVICE, "RCCL (librccl.so) could not be loaded");
    Device& d = c->devs[0];
    HIPCHK(c, hipSetDevice(d.id));
    if (d.comm) {
        (void)rccl().CommDestroy(d.comm);
        d.comm = nullptr;
    }
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    const Clock::time_point deadline = comm_deadline(c);
    if (rccl().CommInitRankConfig && rccl().CommGetAsyncError && rccl().CommAbort) {
        // non-blocking: ncclCommInitRankConfig returns at once and the init is polled against the
        // deadline, so a rank that never joins cannot hold this one
        ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
        cfg.blocking = 0;
        const ncclResult_t e = rccl().CommInitRankConfig(&d.comm, world, uid, rank, &cfg);
        if (e != ncclSuccess && e != ncclInProgress) {
            if (d.comm) (void)rccl().CommAbort(d.comm);
            d.comm = nullptr;
            return set_err(c, RT_ERR_DEVICE, std::string("ncclCommInitRankConfig: ") + rccl().GetErrorString(e));
        }
        c->comm_nonblocking = true;
        c->proc_comm = true;
        const int r = comm_wait(c, d.comm, deadline, "ncclCommInitRankConfig");
        if (r) return r;
    } else {
        NCCLCHK(c, rccl().CommInitRank(&d.comm, world, uid, rank));
        c->comm_nonblocking = false;
        c->proc_comm = true;
    }
    return RT_OK;
}

int rt_comm_set_timeout(rt_ctx* c, int timeout_ms) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (timeout_ms < 0) return set_err(c, RT_ERR_INVALID_ARG, "rt_comm_set_timeout: negative timeout");
    c->comm_timeout_ms = timeout_ms;
    return RT_OK;
}

int rt_comm_abort(rt_ctx* c) {
    if (!c) return RT_ERR_INVALID_ARG;
    abort_comms(c);
    return RT_OK;
}

int rt_gather_image(rt_ctx* c, float* rgba) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (c->width <= 0) return set_err(c, RT_ERR_STATE, "no image");
    if (c->devs.size() != 1) {   // a multi-device context gathers in rt_read_image
        if (!rgba) return set_err(c, RT_ERR_INVALID_ARG, "NULL image");
        return rt_read_image(c, rgba);
    }
    Device& d = c->devs[0];
    if (!c->proc_comm || !d.comm) return set_err(c, RT_ERR_STATE, "rt_comm_init before rt_gather_image");
    if (c->proc_rank == 0 && !rgba) return set_err(c, RT_ERR_INVALID_ARG, "rank 0 needs the output image");
    int r = rt_sync(c);
    if (r) return r;
    HIPCHK(c, hipSetDevice(d.id));
    const int world = c->proc_world;
    // every wait below ends by the context's deadline (rt_comm_set_timeout): on a non-blocking
    // communicator the enqueue is polled (comm_wait), and the stream is polled, not synchronised
    const Clock::time_point deadline = comm_deadline(c);
    // rank k sends its local_rows x W block (a bound image holds no more); rank 0 receives
    // it into slot k of the padded gather buffer
    const size_t slot = (size_t)d.padded_rows * c->width * 16;
    if (c->proc_rank == 0) {
        if (ensure(c, d, d.gather, slot * world) || ensure(c, d, d.full, (size_t)c->height * c->width * 16))
            return RT_ERR_DEVICE;
        NCCLCHK(c, rccl().GroupStart());
        int in_group = group_body(c, [&]() -> int {
            HIPCHK(c, hipMemcpyAsync(d.gather.ptr, d.image_ptr, (size_t)d.local_rows * c->width * 16,
                                     hipMemcpyDeviceToDevice, d.stream));
            for (int k = 1; k < world; k++) {
                const size_t nk = (size_t)local_rows_of(c->height, k, world, c->stripe_rows) * c->width * 4;
                if (nk)
                    NCCLCHK(c, rccl().Recv((char*)d.gather.ptr + slot * k, nk, ncclFloat, k, d.comm, d.stream));
            }
            return RT_OK;
        });
        if (in_group) return in_group;
        if ((r = comm_wait(c, d.comm, deadline, "ncclRecv group"))) return r;
        if (rt_launch_deinterleave(d.gather.ptr, d.full.ptr, c->width, c->height, world, c->stripe_rows,
                                   d.padded_rows, d.stream))
            return set_err(c, RT_ERR_DEVICE, "de-interleave kernel launch failed");
        if ((r = stream_wait(c, d, deadline, "ncclRecv"))) return r;
        if ((r = d2h(c, d, rgba, d.full.ptr, (size_t)c->height * c->width * 16))) return r;
    } else {
        const size_t n = (size_t)d.local_rows * c->width * 4;
        if (n) {
            ncclResult_t e = rccl().Send(d.image_ptr, n, ncclFloat, 0, d.comm, d.stream);
            if (e == ncclInProgress && c->comm_nonblocking) e = ncclSuccess;
            if (e != ncclSuccess) {   // a failed Send frees the communicator too
                abort_comms(c);
                return set_err(c, RT_ERR_DEVICE, std::string("ncclSend: ") + rccl().GetErrorString(e));
            }
            if ((r = comm_wait(c, d.comm, deadline, "ncclSend"))) return r;
        }
        if ((r = stream_wait(c, d, deadline, "ncclSend"))) return r;
    }
    c->gather_path = RT_GATHER_RCCL;
    return RT_OK;
}

int rt_gather_path(rt_ctx* c) { return c ? c->gather_path : RT_ERR_INVALID_ARG; }

}  // extern "C"
