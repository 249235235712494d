// rg_api_comm.cpp -- the sharded path behind the C-ABI: compact records, the RCCL loader, the gather and its expansion.
#include <dlfcn.h>

#include <cstring>
#include <mutex>

#include "rg_handle.h"
#include "rg_launch.h"

// The few RCCL declarations this file needs, spelled out: librccl is bound with dlopen at run time, so building the single-GPU library must not
// need the RCCL development headers either.  (ABI of nccl.h / rccl.h 2.x: ncclUniqueId = 128 opaque bytes passed by value, ncclComm_t an opaque
// pointer (rg_handle.h), ncclSuccess = 0, ncclUint8 = 1.)
extern "C" {
typedef struct { char internal[128]; } ncclUniqueId;
typedef int ncclResult_t;
typedef int ncclDataType_t;
}
static const ncclResult_t ncclSuccess = 0;
static const ncclDataType_t ncclUint8 = 1;

extern "C" {
int rg_compact_record_bytes(const rg_t *h, int with_hist) { return h->S.hw + RG_COMPACT_FIXED_BYTES + (with_hist ? h->S.hw : 0); }

int rg_pack_compact(rg_t *h, int with_hist, uint8_t *out_dev) {
    if (refuse_mixed(h, "rg_pack_compact")) return 1;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->S.hw & 3) { h->err = "rg_pack_compact needs H*W divisible by 4"; return 1; }
    if (flush_mirrors(h)) return 1;
    rgk_pack(&h->S, with_hist ? 1 : 0, out_dev, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The one collective of the sharded path behind the C-ABI: RCCL over xGMI.  librccl is bound at run time (dlopen on first use):
// a single-GPU user of this library needs no RCCL, and inside a PyTorch process the soname resolves to the copy torch already loaded, so
// there is one RCCL per process.
// ---------------------------------------------------------------------------------------------
namespace {
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;  // optional
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;     // optional (rg_comm_count)
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;  // optional
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
};
Rccl *rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
        }
        if (!r.lib) { r.err = std::string("librccl not found: ") + dlerror(); return; }
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
        r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(r.lib, "ncclAllGather"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
        r.CommAbort = reinterpret_cast<decltype(r.CommAbort)>(dlsym(r.lib, "ncclCommAbort"));
        r.CommCount = reinterpret_cast<decltype(r.CommCount)>(dlsym(r.lib, "ncclCommCount"));
        r.CommUserRank = reinterpret_cast<decltype(r.CommUserRank)>(dlsym(r.lib, "ncclCommUserRank"));
        if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy || !r.GetErrorString) r.err = "librccl lacks an expected symbol";
    });
    return &r;
}
}  // namespace

int rg_comm_unique_id(uint8_t id[128]) {
    Rccl *r = rccl();
    if (!r->err.empty()) { g_create_err = r->err; return 1; }
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId");
    ncclUniqueId u;
    ncclResult_t e = r->GetUniqueId(&u);
    if (e != ncclSuccess) { g_create_err = std::string("ncclGetUniqueId: ") + r->GetErrorString(e); return 1; }
    memcpy(id, &u, 128);
    return 0;
}

int rg_comm_init(rg_t *h, const uint8_t id[128], int rank, int world) {
    Rccl *r = rccl();
    if (!r->err.empty()) { h->err = r->err; return 1; }
    if (world < 1 || rank < 0 || rank >= world) { h->err = "rg_comm_init: invalid rank / world"; return 1; }
    if (h->comm) { h->err = "rg_comm_init: the handle already has a communicator"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    ncclUniqueId u;
    memcpy(&u, id, 128);
    ncclResult_t e = r->CommInitRank(&h->comm, world, u, rank);
    if (e != ncclSuccess) { h->comm = nullptr; h->err = std::string("ncclCommInitRank: ") + r->GetErrorString(e); return 1; }
    h->comm_rank = rank; h->comm_world = world;
    return 0;
}

// teardown (rg_destroy): ncclCommAbort where the library has it -- ncclCommDestroy may block when peer ranks have already exited
int comm_release(rg_handle *h, bool teardown) {
    if (!h->comm) return 0;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    Rccl *r = rccl();
    ncclResult_t e = (teardown && r->CommAbort) ? r->CommAbort(h->comm) : r->CommDestroy(h->comm);
    h->comm = nullptr; h->comm_world = 1; h->comm_rank = 0;
    if (e != ncclSuccess) { h->err = std::string("ncclCommDestroy: ") + r->GetErrorString(e); return 1; }
    return 0;
}
int rg_comm_destroy(rg_t *h) { return comm_release(h, false); }

// What the COMMUNICATOR says about itself (ncclCommCount / ncclCommUserRank), not what rg_comm_init was told: the proof that RCCL saw `world` ranks.
int rg_comm_count(rg_t *h, int *count, int *rank) {
    if (!h->comm) { h->err = "rg_comm_count: no communicator (rg_comm_init first)"; return 1; }
    Rccl *r = rccl();
    if (!r->CommCount || !r->CommUserRank) { h->err = "rg_comm_count: librccl lacks ncclCommCount / ncclCommUserRank"; return 1; }
    int c = 0, u = 0;
    ncclResult_t e = r->CommCount(h->comm, &c);
    if (e == ncclSuccess) e = r->CommUserRank(h->comm, &u);
    if (e != ncclSuccess) { h->err = std::string("ncclCommCount: ") + r->GetErrorString(e); return 1; }
    if (count) *count = c;
    if (rank) *rank = u;
    return 0;
}

int rg_allgather_compact(rg_t *h, int with_hist, uint8_t *out_dev) {
    if (!h->comm) { h->err = "rg_allgather_compact: no communicator (rg_comm_init first)"; return 1; }
    const size_t bytes = (size_t)h->S.n * (size_t)rg_compact_record_bytes(h, with_hist);
    // pack straight into this rank's slice of the gathered batch, then gather IN PLACE (sendbuff == recvbuff + rank * count) on the handle's stream:
    // no staging copy, and the collective is ordered behind the step like any other launch of the handle
    uint8_t *mine = out_dev + (size_t)h->comm_rank * bytes;
    if (rg_pack_compact(h, with_hist, mine)) return 1;
    ncclResult_t e = rccl()->AllGather(mine, out_dev, bytes, ncclUint8, h->comm, h->stream);
    if (e != ncclSuccess) { h->err = std::string("ncclAllGather: ") + rccl()->GetErrorString(e); return 1; }
    return 0;
}

int rg_expand_compact(rg_t *h, const uint8_t *packed_dev, int n, int packed_has_hist, int kind, uint32_t status_flag, int with_hist, float *out_dev) {
    if (refuse_mixed(h, "rg_expand_compact")) return 1;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->S.hw & 3) { h->err = "rg_expand_compact needs H*W divisible by 4"; return 1; }
    if (with_hist && !packed_has_hist) { h->err = "rg_expand_compact: the packed batch carries no history plane"; return 1; }
    const size_t hw = (size_t)h->S.hw, rec = hw + RG_COMPACT_FIXED_BYTES + (packed_has_hist ? hw : 0);
    rgk_encode(packed_dev, packed_dev + RG_COMPACT_HIST_OFFSET(hw), reinterpret_cast<const int32_t *>(packed_dev + RG_COMPACT_STATUS_OFFSET(hw)), nullptr, h->d_err, n, (int)hw, rec, rec / 4, h->cfg.symbols,
               h->cfg.symbols, status_flag & 0x1ffu, with_hist ? 1 : 0, kind, out_dev, nullptr, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}
}  // extern "C"
