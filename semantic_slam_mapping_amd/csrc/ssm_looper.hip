// ssm_looper.hip -- rgbd_tutor::Looper (reference include/looper.h, src/looper.cpp) behind the C ABI: the device looper of a context (kernels_bow.hip) over a
// vocabulary (a host object: ssm_vocab.cpp): a CSR database of bag-of-words vectors that grows by doubling, bulk add from device descriptors, score rows
// and ordered loop candidates.
#include "ssm_ctx.h"
#include "ssm_host.h"

// ---------------------------------------------------------------- the device looper
struct ssm_looper {
    ssm_ctx* c = nullptr;
    int cap = 0, P = 0, variant = 0;                      // features per frame at most (ssm_orb_capacity), its power of two, the descent kernel
    // the vocabulary on the device
    DevBuf<int32_t> d_first, d_nchild, d_word; DevBuf<uint32_t> d_desc; DevBuf<double> d_weight; ssm_bow::Tree tree{};
    // the database: entry e = offsets[e] .. offsets[e + 1] of (ids, vals); frame_ids[e]
    DevBuf<int32_t> d_offsets, d_ids, d_frame_ids; DevBuf<double> d_vals; DevBuf<int32_t> d_hdr;
    PinBuf<int32_t> h_frame_ids;                          // the frame ids again, page-locked: the upload of an add reads them after the call has returned
    int entries = 0, entry_cap = 0; long long nnz_ub = 0, nnz_cap = 0;      // nnz_ub: what the host knows the entries hold at most
    // staging of one add (frames x cap) and of one query
    DevBuf<uint8_t> d_in; DevBuf<int32_t> d_words, d_st_ids, d_st_m; DevBuf<double> d_st_vals; int stage_frames = 0;
    DevBuf<double> d_scores, d_out_scores; DevBuf<int32_t> d_counts, d_pairs; size_t scores_n = 0; int counts_n = 0, out_n = 0;
};
#define LFAIL(l, code, msg) do { (l)->c->err = (msg); return (code); } while (0)
template <class T> static int grow_keep(ssm_looper* l, DevBuf<T>& b, size_t keep, size_t count)      // b <- a buffer of `count` elements that starts with b's first `keep`
{
    ssm_ctx* c = l->c;
    DevBuf<T> nb; { const int r = nb.alloc(c, count); if (r) return r; }
    if (keep) HIPCHK(c, hipMemcpyAsync(nb, b, keep * sizeof(T), hipMemcpyDeviceToDevice, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));             // the old buffer goes: nothing queued may still read it
    b = std::move(nb);
    return SSM_OK;
}
// room for `add_entries` more entries holding at most `add_nnz` values.  The exact fill is only known on the device; the host tracks an upper bound and asks
// for the exact number (one wait) only when the bound does not fit
static int looper_reserve(ssm_looper* l, int add_entries, long long add_nnz)
{
    ssm_ctx* c = l->c;
    if (l->entries + add_entries > l->entry_cap) {
        int nc = l->entry_cap ? l->entry_cap : 256; while (nc < l->entries + add_entries) nc *= 2;
        { const int r = grow_keep(l, l->d_offsets, l->entry_cap ? (size_t)l->entries + 1 : 0, (size_t)nc + 1); if (r) return r; }
        { const int r = grow_keep(l, l->d_frame_ids, l->entry_cap ? (size_t)l->entries : 0, (size_t)nc); if (r) return r; }
        { PinBuf<int32_t> nh; const int r = nh.alloc(c, (size_t)nc); if (r) return r;            // (grow_keep has drained the stream: no copy still reads the old block)
          if (l->entries) memcpy(nh, l->h_frame_ids, (size_t)l->entries * 4);
          l->h_frame_ids = std::move(nh); }
        if (!l->entry_cap) HIPCHK(c, hipMemsetAsync(l->d_offsets, 0, 4, c->main.stream));
        l->entry_cap = nc;
    }
    if (l->nnz_ub + add_nnz > l->nnz_cap) {
        int32_t exact = 0;
        if (l->entries) { HIPCHK(c, hipMemcpyAsync(&exact, l->d_offsets + l->entries, 4, hipMemcpyDeviceToHost, c->main.stream)); HIPCHK(c, hipStreamSynchronize(c->main.stream)); }
        l->nnz_ub = exact;
        if (l->nnz_ub + add_nnz > 0x7FFFFFFFll) LFAIL(l, SSM_E_CAPACITY, "looper: the database would exceed 2^31 values");
        if (l->nnz_ub + add_nnz > l->nnz_cap) {
            long long nc = l->nnz_cap ? l->nnz_cap : 1 << 16; while (nc < l->nnz_ub + add_nnz) nc *= 2;
            { const int r = grow_keep(l, l->d_ids, (size_t)l->nnz_ub, (size_t)nc); if (r) return r; }
            { const int r = grow_keep(l, l->d_vals, (size_t)l->nnz_ub, (size_t)nc); if (r) return r; }
            l->nnz_cap = nc;
        }
    }
    return SSM_OK;
}
static int looper_stage(ssm_looper* l, int frames)
{
    ssm_ctx* c = l->c;
    if (frames <= l->stage_frames) return SSM_OK;
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    int nf = l->stage_frames ? l->stage_frames : 1; while (nf < frames) nf *= 2;
    const size_t n = (size_t)nf * l->cap;
    DALLOC(c, l->d_words, n); DALLOC(c, l->d_st_ids, n); DALLOC(c, l->d_st_vals, n); DALLOC(c, l->d_st_m, nf);
    l->stage_frames = nf;
    return SSM_OK;
}
// the frames' descriptors are on the device (desc_dev: frames x cap x 32; nkp_dev, or every frame has n_fixed): words -> vectors -> database, all enqueued
static int looper_add_enqueue(ssm_looper* l, const uint8_t* desc_dev, const int32_t* nkp_dev, int n_fixed, int frames, const int32_t* frame_ids, long long nnz_bound)
{
    ssm_ctx* c = l->c;
    { const int r = looper_reserve(l, frames, nnz_bound); if (r) return r; }
    { const int r = looper_stage(l, frames); if (r) return r; }
    memcpy(l->h_frame_ids + l->entries, frame_ids, (size_t)frames * 4);
    HIPCHK(c, hipMemcpyAsync(l->d_frame_ids + l->entries, l->h_frame_ids + l->entries, (size_t)frames * 4, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, k_bow_words(l->tree, desc_dev, nkp_dev, n_fixed, frames, l->cap, l->d_words, l->variant, c->main.stream));
    HIPCHK(c, k_bow_frame(l->d_words, l->d_weight, nkp_dev, n_fixed, frames, l->cap, l->P, l->d_st_ids, l->d_st_vals, l->d_st_m, c->main.stream));
    HIPCHK(c, k_bow_append(l->d_st_ids, l->d_st_vals, l->d_st_m, frames, l->cap, l->d_offsets, l->entries, l->d_ids, l->d_vals, l->nnz_cap, l->d_hdr, c->main.stream));
    l->entries += frames; l->nnz_ub += nnz_bound;
    return SSM_OK;
}

extern "C" int ssm_looper_create(ssm_ctx* c, const ssm_vocab* v, ssm_looper** out)
{
    if (!c || !out) return SSM_E_INVAL;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (!v) FAIL(c, SSM_E_INVAL, "looper: null vocabulary");
    const int cap = c->g.cap;
    if (cap < 1 || cap > 4096) FAIL(c, SSM_E_INVAL, "looper: at most 4096 features per frame (ssm_orb_capacity)");
    std::unique_ptr<ssm_looper> l(new ssm_looper());
    l->c = c; l->cap = cap; l->P = 2; while (l->P < cap) l->P *= 2;
    { const char* e = getenv("SSM_BOW_VARIANT"); l->variant = (e && atoi(e) == 1) ? 1 : 0; }        // 1: one lane per descriptor (ablation runs); default: 16 lanes per descriptor
    const size_t nn = v->n_child.size(), nw = v->weight.size();
    DALLOC(c, l->d_first, nn); DALLOC(c, l->d_nchild, nn); DALLOC(c, l->d_word, nn); DALLOC(c, l->d_desc, nn * 8); DALLOC(c, l->d_weight, nw); DALLOC(c, l->d_hdr, 4);
    HIPCHK(c, hipMemcpyAsync(l->d_first, v->first_child.data(), nn * 4, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(l->d_nchild, v->n_child.data(), nn * 4, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(l->d_word, v->word.data(), nn * 4, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(l->d_desc, v->desc.data(), nn * 32, hipMemcpyHostToDevice, c->main.stream));
    if (nw) HIPCHK(c, hipMemcpyAsync(l->d_weight, v->weight.data(), nw * 8, hipMemcpyHostToDevice, c->main.stream));
    HIPCHK(c, hipMemsetAsync(l->d_hdr, 0, 16, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));             // v may be destroyed once this returns
    l->tree.first_child = l->d_first; l->tree.n_child = l->d_nchild; l->tree.desc = l->d_desc; l->tree.word = l->d_word; l->tree.weight = l->d_weight;
    l->tree.n_nodes = (int)nn; l->tree.n_words = (int)nw; l->tree.max_depth = v->max_depth;
    *out = l.release();
    return SSM_OK;
}
extern "C" void ssm_looper_destroy(ssm_looper* l)
{
    if (!l) return;
    { std::lock_guard<std::mutex> lk(l->c->mu); hipSetDevice(l->c->device); (void)hipStreamSynchronize(l->c->main.stream); }
    delete l;
}
extern "C" int ssm_looper_clear(ssm_looper* l)
{
    if (!l) return SSM_E_INVAL;
    ssm_ctx* c = l->c; std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    l->entries = 0; l->nnz_ub = 0;
    if (l->entry_cap) HIPCHK(c, hipMemsetAsync(l->d_offsets, 0, 4, c->main.stream));
    return SSM_OK;
}
extern "C" int ssm_looper_size(const ssm_looper* l) { return l ? l->entries : 0; }
// the overflow word of the append kernel, after the stream has been waited for
static int looper_check(ssm_looper* l, const int32_t* hdr) { if (hdr[0]) LFAIL(l, SSM_E_CAPACITY, "looper: the database overflowed its reservation"); return SSM_OK; }

extern "C" int ssm_looper_add(ssm_looper* l, const uint8_t* desc, int n, int frame_id)
{
    if (!l) return SSM_E_INVAL;
    ssm_ctx* c = l->c; std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (n < 0 || (n > 0 && !desc)) FAIL(c, SSM_E_INVAL, "bad arguments");
    if (n > l->cap) FAIL(c, SSM_E_CAPACITY, "looper: more descriptors than ssm_orb_capacity");
    if (l->d_in.bytes() < (size_t)l->cap * 32) DALLOC(c, l->d_in, (size_t)l->cap * 32);
    if (n) HIPCHK(c, hipMemcpyAsync(l->d_in, desc, (size_t)n * 32, hipMemcpyHostToDevice, c->main.stream));
    const int32_t fid = frame_id;
    { const int r = looper_add_enqueue(l, l->d_in, nullptr, n, 1, &fid, n); if (r) return r; }
    int32_t hdr[4];
    HIPCHK(c, hipMemcpyAsync(hdr, l->d_hdr, 16, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return looper_check(l, hdr);
}
extern "C" int ssm_looper_add_dev(ssm_looper* l, const uint8_t* desc_dev, const int32_t* nkp_dev, int n_frames, int cap, const int32_t* frame_ids)
{
    if (!l) return SSM_E_INVAL;
    ssm_ctx* c = l->c; std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (n_frames < 0 || (n_frames > 0 && (!desc_dev || !nkp_dev || !frame_ids))) FAIL(c, SSM_E_INVAL, "bad arguments");
    if (cap != l->cap) FAIL(c, SSM_E_INVAL, "looper: cap must be the context's ssm_orb_capacity (the layout of ssm_seq_out_dev.desc)");
    if (n_frames == 0) return SSM_OK;
    return looper_add_enqueue(l, desc_dev, nkp_dev, 0, n_frames, frame_ids, (long long)n_frames * l->cap);
}
extern "C" int ssm_looper_bow(ssm_looper* l, int entry, int32_t* ids, double* vals, int cap, int* n_out)
{
    if (!l) return SSM_E_INVAL;
    ssm_ctx* c = l->c; std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (entry < 0 || entry >= l->entries || !n_out || cap < 0 || (cap > 0 && (!ids || !vals))) FAIL(c, SSM_E_INVAL, "bad arguments");
    int32_t o[2], hdr[4];
    HIPCHK(c, hipMemcpyAsync(o, l->d_offsets + entry, 8, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(hdr, l->d_hdr, 16, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    { const int r = looper_check(l, hdr); if (r) return r; }
    const int m = o[1] - o[0];
    *n_out = m;
    if (m > cap) FAIL(c, SSM_E_CAPACITY, "looper: the vector has more entries than the caller's buffers");
    if (m) {
        HIPCHK(c, hipMemcpyAsync(ids, l->d_ids + o[0], (size_t)m * 4, hipMemcpyDeviceToHost, c->main.stream));
        HIPCHK(c, hipMemcpyAsync(vals, l->d_vals + o[0], (size_t)m * 8, hipMemcpyDeviceToHost, c->main.stream));
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
    }
    return SSM_OK;
}
// score rows of the query entries [first, first + n) + their candidate counts, enqueued; row = entries per row
static int looper_scores_enqueue(ssm_looper* l, int first, int n, int against, double min_score, int min_interval, int* row_out)
{
    ssm_ctx* c = l->c;
    const int row = against < 0 ? first + n : against;
    const size_t need = (size_t)n * (row ? row : 1);
    if (need > l->scores_n || n > l->counts_n) {
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
        if (need > l->scores_n) { DALLOC(c, l->d_scores, need); l->scores_n = need; }
        if (n > l->counts_n) { DALLOC(c, l->d_counts, n); l->counts_n = n; }
    }
    HIPCHK(c, k_bow_score(l->d_offsets, l->d_ids, l->d_vals, l->d_frame_ids, first, n, against, row, l->cap, min_score, min_interval, l->d_scores, l->d_counts, c->main.stream));
    *row_out = row;
    return SSM_OK;
}
extern "C" int ssm_looper_scores(ssm_looper* l, int entry, int against, double* scores)
{
    if (!l) return SSM_E_INVAL;
    ssm_ctx* c = l->c; std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (entry < 0 || entry >= l->entries || against < -1 || against > l->entries || !scores) FAIL(c, SSM_E_INVAL, "bad arguments");
    int row = 0;
    { const int r = looper_scores_enqueue(l, entry, 1, against, 0.0, 0, &row); if (r) return r; }
    int32_t hdr[4];
    if (row) HIPCHK(c, hipMemcpyAsync(scores, l->d_scores, (size_t)row * 8, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipMemcpyAsync(hdr, l->d_hdr, 16, hipMemcpyDeviceToHost, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return looper_check(l, hdr);
}
extern "C" int ssm_looper_query(ssm_looper* l, int first, int n, int against, double min_sim_score, int min_interval, int32_t* pairs, double* scores, int cap, int* n_out)
{
    if (!l) return SSM_E_INVAL;
    ssm_ctx* c = l->c; std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
    if (first < 0 || n < 0 || first + n > l->entries || against < -1 || against > l->entries || !n_out || cap < 0 || (cap > 0 && (!pairs || !scores))) FAIL(c, SSM_E_INVAL, "bad arguments");
    *n_out = 0;
    if (n == 0) return SSM_OK;
    int row = 0;
    { const int r = looper_scores_enqueue(l, first, n, against, min_sim_score, min_interval, &row); if (r) return r; }
    // the output is staged for min(cap, every pair) candidates, so that count and candidates come back with one wait
    long long all = against < 0 ? (long long)n * first + (long long)n * (n + 1) / 2 : (long long)n * against;
    const int stage = (int)std::min<long long>(cap, all);
    if (stage > l->out_n) {
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
        DALLOC(c, l->d_pairs, (size_t)stage * 2); DALLOC(c, l->d_out_scores, stage); l->out_n = stage;
    }
    HIPCHK(c, k_bow_emit(l->d_frame_ids, l->d_scores, l->d_counts, first, n, against, row, min_sim_score, min_interval, l->d_pairs, l->d_out_scores, stage, l->d_hdr, c->main.stream));
    int32_t hdr[4];
    HIPCHK(c, hipMemcpyAsync(hdr, l->d_hdr, 16, hipMemcpyDeviceToHost, c->main.stream));
    if (stage) {
        HIPCHK(c, hipMemcpyAsync(pairs, l->d_pairs, (size_t)stage * 8, hipMemcpyDeviceToHost, c->main.stream));
        HIPCHK(c, hipMemcpyAsync(scores, l->d_out_scores, (size_t)stage * 8, hipMemcpyDeviceToHost, c->main.stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    { const int r = looper_check(l, hdr); if (r) return r; }
    *n_out = hdr[1];
    if (hdr[1] > cap) FAIL(c, SSM_E_CAPACITY, "looper: more candidates than the caller's buffers hold");
    return SSM_OK;
}
