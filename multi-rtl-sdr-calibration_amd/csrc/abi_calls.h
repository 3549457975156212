// abi_calls.h -- the C ABI entry points of include/gsmcal.h for the DSP chain: context, parameters, the per-function
// MATLAB-signature calls (a1..a9, f4) and the batched hot path.  Included by gsmcal.hip inside its extern "C" block.
#pragma once

const char* gsmcal_version(void) { return GSMCAL_VERSION; }

void gsmcal_params_default(gsmcal_params* p) {
    if (!p) return;
    p->coarse_th_db = 10.0; p->coarse_mv_factor = 10; p->coarse_max_offset = 5; p->min_hits = 5;
    p->fine_max_offset = 64; p->fine_max_ppm = 4000.0; p->fine_gate_snr_db = 5.0; p->fine_noise_bw_hz = 200e3;
    p->sch_max_offset = 8; p->sch_max_ppm = 400.0; p->post_min_bcch = 4;
    p->scan_min_hits = 3; p->scan_spacing = 12500.0; p->scan_spacing_idle = 12500.0 + 1250.0; p->scan_tol = 50.0;
}

int gsmcal_set_params(gsmcal_ctx* c, const gsmcal_params* p) {
    if (!c || !p) return GSMCAL_E_ARG;
    RET_IF(pipe_join(c));
    gsmcal_params d;
    gsmcal_params_default(&d);
    if (p->coarse_mv_factor != d.coarse_mv_factor || p->coarse_max_offset != d.coarse_max_offset ||
        p->fine_max_offset != d.fine_max_offset || p->fine_noise_bw_hz != d.fine_noise_bw_hz || p->sch_max_offset != d.sch_max_offset) {
        c->err = "gsmcal_set_params: a geometry field differs from its default";
        return GSMCAL_E_UNSUPPORTED;
    }
    if (p->min_hits < 2 || p->min_hits > GSMCAL_MAX_HITS || p->scan_min_hits < 1 || p->post_min_bcch < 0) {
        c->err = "gsmcal_set_params: min_hits outside 2..GSMCAL_MAX_HITS, scan_min_hits < 1 or post_min_bcch < 0";
        return GSMCAL_E_ARG;
    }
    // every comparison with a NaN threshold is false: the coarse detector would never hit and its certificate never decide, the
    // spacing classes would be empty, the SNR gate open -- no caller means that; refused rather than defined
    if (std::isnan(p->coarse_th_db) || std::isnan(p->fine_max_ppm) || std::isnan(p->fine_gate_snr_db) || std::isnan(p->sch_max_ppm) ||
        std::isnan(p->scan_spacing) || std::isnan(p->scan_spacing_idle) || std::isnan(p->scan_tol)) {
        c->err = "gsmcal_set_params: a threshold is NaN";
        return GSMCAL_E_ARG;
    }
    c->params = *p;
    ++c->params_epoch;
    return 0;
}

int gsmcal_get_params(gsmcal_ctx* c, gsmcal_params* p) {
    if (!c || !p) return GSMCAL_E_ARG;
    *p = c->params;
    return 0;
}

int gsmcal_ctx_create_on_stream(int device_id, void* hip_stream, gsmcal_ctx** out) {
    if (!out) return GSMCAL_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GSMCAL_E_NO_DEVICE;
    if (device_id < 0 || device_id >= n) return GSMCAL_E_ARG;
    if (hipSetDevice(device_id) != hipSuccess) return GSMCAL_E_HIP;
    // kernels whose dynamic LDS may exceed the 64 KiB default
    (void)hipFuncSetAttribute((const void*)k_gather, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)k_fir_decim_raw, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_fine_verify, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_fine_cert<0, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_fine_cert<8, 47>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_fine_chunk, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_front_fused, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_front_fast47_sym, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_front_fast47, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_front_fast31_sym, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_front_fast31, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_coarse_scan_lat, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_coarse_scan_inl, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_coarse_scan_gen, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_coarse_scan_ref, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_burst_tone<0, 0, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_burst_tone<1, 0, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_window_sch<0, 0, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_post_chain_r<0, 0, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_post_chain_r<8, 512, 47>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_sch_equalise, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_sch_fd_training, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_fcch_demod, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_fft_burst<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_fft_burst<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_burst_tone<0, 8, 47>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_burst_tone<1, 8, 47>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipFuncSetAttribute((const void*)k_window_sch<8, 512, 47>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipGetLastError();   // an attribute request the device rejects must not surface at the first launch
    gsmcal_ctx* c = new gsmcal_ctx();
    gsmcal_params_default(&c->params);
    c->device = device_id;
    c->stream = (hipStream_t)hip_stream;
    c->own_stream = false;
    c->lanes[0].stream = c->stream;
    c->cur = &c->lanes[0];
    const char* e = getenv("GSMCAL_LANES");
    if (e && atoi(e) >= 1) c->n_lanes_cfg = atoi(e) > MAX_LANES ? MAX_LANES : atoi(e);
    { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && ncu > 0) c->n_cu = ncu; }
    { int lds = 0; if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, c->device) == hipSuccess && lds > 0) c->lds_per_cu = (size_t)lds; }
    if (const char* e2 = getenv("GSMCAL_SNR_INLINE_MIN")) c->snr_inline_min = atoi(e2);
    if (const char* e2 = getenv("GSMCAL_SNR_INLINE_KEEP")) c->snr_inline_keep = atoi(e2);
    if (const char* e2 = getenv("GSMCAL_FRONT_NT")) c->front_nt = atoi(e2);
    if (const char* e2 = getenv("GSMCAL_SCAN_SPLIT")) c->scan_split = atoi(e2);
    const char* sst = getenv("GSMCAL_SCAN_STAGES");
    if (sst && atoi(sst) >= 1) c->scan_stages = atoi(sst);
    const char* lm = getenv("GSMCAL_LANE_MIN");
    if (lm && atoi(lm) >= 1) c->lane_min = atoi(lm);
    const char* ce = getenv("GSMCAL_CERT");
    if (ce) c->certify = atoi(ce) != 0;
    const char* sfe = getenv("GSMCAL_SNR_FULL");
    if (sfe) c->snr_full = atoi(sfe) != 0;
    const char* sse = getenv("GSMCAL_SNR_SCREEN_DB");
    if (sse) c->snr_screen_db = atof(sse);
    const char* fge = getenv("GSMCAL_FUSE_GATHER");
    if (fge) c->fuse_fine_gather = atoi(fge) != 0;
    const char* fpe = getenv("GSMCAL_FUSE_POST");
    if (fpe) c->fuse_post = atoi(fpe) != 0;
    const char* pse = getenv("GSMCAL_POST_SLOTS");
    if (pse && atoi(pse) >= 1) c->post_slots_cap = atoi(pse);
    const char* pe = getenv("GSMCAL_PRESCREEN");
    if (pe && atoi(pe) == 0) c->prescreen = false;
    const char* fg = getenv("GSMCAL_FRONT_GENERIC");
    if (fg && atoi(fg) != 0) c->front_generic = true;
    if (const char* e2 = getenv("GSMCAL_FUSED_POLL_S")) { if (atof(e2) > 0.0) c->fused_poll_s = atof(e2); }
    if (const char* e2 = getenv("GSMCAL_TEST_FUSED_STALL")) c->test_stall = atoi(e2);
    const char* ge = getenv("GSMCAL_GRAPH");
    if (ge && atoi(ge) == 0) c->use_graph = false;
    if (ge && atoi(ge) == 2) c->graph_always = true;
    fused_gate_register(c);
    *out = c;
    return 0;
}

int gsmcal_ctx_create(int device_id, gsmcal_ctx** out) {
    int r = gsmcal_ctx_create_on_stream(device_id, nullptr, out);
    if (r != 0) return r;
    gsmcal_ctx* c = *out;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        fused_gate_unregister(c);
        delete c;
        *out = nullptr;
        return GSMCAL_E_HIP;
    }
    c->own_stream = true;
    c->lanes[0].stream = c->stream;
    return 0;
}

void gsmcal_ctx_destroy(gsmcal_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)pipe_drain(c);
    (void)hipStreamSynchronize(c->stream);
    (void)hipDeviceSynchronize();
    fused_gate_unregister(c);
    const auto free_buf = [](DevBuf& b) { if (b.p) (void)hipFree(b.p); };
    c->for_each_buf(free_buf);
    for (int i = 0; i < MAX_LANES; ++i) {
        Lane& L = c->lanes[i];
        L.for_each_buf(free_buf);
        if (L.done) (void)hipEventDestroy(L.done);
        if (L.front_done) (void)hipEventDestroy(L.front_done);
        if (i > 0 && L.stream) (void)hipStreamDestroy(L.stream);
    }
    for (int i = 0; i < gsmcal_ctx::PIPE_MAX_DEPTH; ++i) {
        c->pipe[i].for_each_buf(free_buf);
        if (c->pipe_done[i]) (void)hipEventDestroy(c->pipe_done[i]);
        if (c->side_in[i]) (void)hipEventDestroy(c->side_in[i]);
    }
    for (hipStream_t st : c->side_owned) (void)hipStreamDestroy(st);
    if (c->fork) (void)hipEventDestroy(c->fork);
    for (hipEvent_t e : c->ag_chain)
        if (e) (void)hipEventDestroy(e);
    if (c->ag_stream) (void)hipStreamSynchronize(c->ag_stream);
    for (int i = 0; i < gsmcal_ctx::AG_SLOTS; ++i) {
        if (c->ag_ready[i]) (void)hipEventDestroy(c->ag_ready[i]);
        if (c->ag_done[i]) (void)hipEventDestroy(c->ag_done[i]);
    }
    if (c->ag_stream) (void)hipStreamDestroy(c->ag_stream);
    for (int i = 0; i < gsmcal_ctx::GRAPH_SLOTS; ++i)
        for (auto* g : {&c->g_calib[i], &c->g_scan[i]}) {
            if (g->exec) (void)hipGraphExecDestroy(g->exec);
            if (g->graph) (void)hipGraphDestroy(g->graph);
        }
    for (auto& r : c->prof_pending) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int gsmcal_fused_tail_stats(gsmcal_ctx* c, unsigned long long* fused_launches, unsigned long long* gate_fallbacks) {
    if (!c) return GSMCAL_E_ARG;
    if (fused_launches) *fused_launches = c->n_fused_launches;
    if (gate_fallbacks) *gate_fallbacks = c->n_gate_fallbacks;
    return 0;
}

// The context's streams have drained.  If a fused tail of the calls since the last check gave up waiting for a peer (the kernel's
// poll limit: another process's fused tail held the slots its workgroups needed), run those calls again -- same inputs, which the
// caller leaves untouched until it has synchronised -- with the four-launch tail, whose kernels wait for nobody.
static int fused_recover(gsmcal_ctx* c) {
    if (!c->fused_done || c->recovering) return 0;
    volatile unsigned* flag = c->fused_done + gsmcal_ctx::FUSED_MAX_STREAMS;
    if (*flag == 0u) { c->fused_calls.clear(); return 0; }
    *flag = 0u;
    std::vector<gsmcal_ctx::FusedCall> calls;
    calls.swap(c->fused_calls);
    const bool fp = c->fuse_post;
    const int depth = c->pipe_depth;
    c->fuse_post = false; c->pipe_depth = 1; c->recovering = true;
    int rc = 0;
    for (auto& k : calls) {
        rc = gsmcal_calibrate_batch_dev(c, k.d_raw, k.d, k.n, k.coef.data(), k.ntaps, k.ts.data(), k.len_ts, k.cf.data(), k.d_table, k.d_pos_info, k.d_r_correct, k.d_r_len);
        if (rc < 0) break;
    }
    hipError_t e = hipSuccess;
    if (rc >= 0) e = hipStreamSynchronize(c->stream);
    c->fuse_post = fp; c->pipe_depth = depth; c->recovering = false;
    ++c->n_tail_reruns;
    if (rc < 0) return rc;
    if (e != hipSuccess) { c->err = std::string("hipStreamSynchronize (fused tail re-run): ") + hipGetErrorString(e); return GSMCAL_E_HIP; }
    return 0;
}

int gsmcal_sync(gsmcal_ctx* c) {
    if (!c) return GSMCAL_E_ARG;
    RET_IF(pipe_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return fused_recover(c);
}

long long gsmcal_fused_tail_reruns(gsmcal_ctx* c) { return c ? (long long)c->n_tail_reruns : (long long)GSMCAL_E_ARG; }

// ---- pipelined batch calls ----------------------------------------------------------------------------------------
int gsmcal_ctx_set_pipeline_depth(gsmcal_ctx* c, int depth) {
    if (!c || depth < 1 || depth > gsmcal_ctx::PIPE_MAX_DEPTH) return GSMCAL_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    RET_IF(pipe_drain(c));
    if (depth > 1) RET_IF(pipe_prepare(c));
    c->pipe_depth = depth;
    return 0;
}

int gsmcal_ctx_get_pipeline_depth(gsmcal_ctx* c) { return c ? c->pipe_depth : GSMCAL_E_ARG; }
int gsmcal_ctx_pipeline_queues(gsmcal_ctx* c) { return c ? c->n_side : GSMCAL_E_ARG; }

const char* gsmcal_last_error(gsmcal_ctx* c) { return c ? c->err.c_str() : "null context"; }

long gsmcal_last_call_report(gsmcal_ctx* c, char* buf, size_t cap) {
    if (!c) return GSMCAL_E_ARG;
    if (buf && cap > 0) {
        const size_t n = c->report.size() < cap - 1 ? c->report.size() : cap - 1;
        memcpy(buf, c->report.data(), n);
        buf[n] = 0;
    }
    return (long)c->report.size();
}

long gsmcal_num2str(const double* x, int n, char* buf, size_t cap) {
    if (!x || n < 0) return GSMCAL_E_ARG;
    const std::string s = rep_num2str(x, n);
    if (buf && cap > 0) {
        const size_t m = s.size() < cap - 1 ? s.size() : cap - 1;
        memcpy(buf, s.data(), m);
        buf[m] = 0;
    }
    return (long)s.size();
}

int gsmcal_dev_alloc(gsmcal_ctx* c, size_t bytes, void** dptr) {
    if (!c || !dptr) return GSMCAL_E_ARG;
    ENTER(c);
    HIPCHK(c, hipMalloc(dptr, bytes));
    return 0;
}
int gsmcal_dev_free(gsmcal_ctx* c, void* dptr) {
    if (!c) return GSMCAL_E_ARG;
    RET_IF(pipe_drain(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(dptr));
    return 0;
}
int gsmcal_memcpy_h2d(gsmcal_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return GSMCAL_E_ARG;
    RET_IF(pipe_join(c));
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int gsmcal_memcpy_d2h(gsmcal_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return GSMCAL_E_ARG;
    RET_IF(pipe_join(c));
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int gsmcal_profile_enable(gsmcal_ctx* c, int enable) {
    if (!c) return GSMCAL_E_ARG;
    RET_IF(pipe_drain(c));
    RET_IF(prof_flush(c));
    c->prof = enable != 0;
    if (c->prof && c->ev_pool.size() < 512) {     // event creation is slow: keep it out of the measured launches
        for (int i = 0; i < 512; ++i) {
            hipEvent_t e;
            if (hipEventCreateWithFlags(&e, hipEventReleaseToDevice) == hipSuccess) c->ev_pool.push_back(e);
        }
    }
    return 0;
}
int gsmcal_profile_filter(gsmcal_ctx* c, const char* substr) {
    if (!c) return GSMCAL_E_ARG;
    c->prof_filter = substr ? substr : "";
    return 0;
}
int gsmcal_profile_reset(gsmcal_ctx* c) {
    if (!c) return GSMCAL_E_ARG;
    RET_IF(prof_flush(c));
    for (auto& v : c->prof_ms) v = 0.0;
    for (auto& v : c->prof_n) v = 0;
    return 0;
}
int gsmcal_profile_get(gsmcal_ctx* c, int cap, const char** names, double* total_ms, long* launches) {
    if (!c) return GSMCAL_E_ARG;
    RET_IF(prof_flush(c));
    const int n = (int)c->prof_names.size();
    for (int i = 0; i < n && i < cap; ++i) {
        if (names) names[i] = c->prof_names[i].c_str();
        if (total_ms) total_ms[i] = c->prof_ms[i];
        if (launches) launches[i] = c->prof_n[i];
    }
    return n;
}

// ---- a1 raw2iq -----------------------------------------------------------------------------------
int gsmcal_raw2iq_u8(gsmcal_ctx* c, const uint8_t* a, long rows_2n, int d, double* b) {
    if (!c || !a || !b || rows_2n < 2 || (rows_2n & 1) || d < 1) return GSMCAL_E_ARG;
    const long n = rows_2n / 2;
    ENTER(c);
    RET_IF(ensure(c, c->misc, (size_t)rows_2n * d));
    RET_IF(ensure(c, c->arr_out, (size_t)n * d * sizeof(cplx)));
    HIPCHK(c, hipMemcpyAsync(c->misc.p, a, (size_t)rows_2n * d, hipMemcpyHostToDevice, c->stream));
    RET_IF(init_states(c, d, n));
    RET_IF(dc_means(c, (const uint8_t*)c->misc.p, d, n));
    int blocks = (int)((n + 256 * 4 - 1) / (256 * 4));
    if (blocks > 2048) blocks = 2048;
    LAUNCH(c, k_raw2iq, dim3(blocks, d), dim3(256), 0, (const uint8_t*)c->misc.p, rows_2n,
           (const StreamState*)c->cur->state.p, (cplx*)c->arr_out.p, n);
    CHECK_LAUNCH(c);
    HIPCHK(c, hipMemcpyAsync(b, c->arr_out.p, (size_t)n * d * sizeof(cplx), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int gsmcal_raw2iq(gsmcal_ctx* c, const double* a, long rows_2n, int d, double* b) {
    if (!c || !a || !b || rows_2n < 2 || (rows_2n & 1) || d < 1) return GSMCAL_E_ARG;
    // the doubles hold byte values (fread(...,'uint8'), gsm_sync_demod.m:96): narrow them back
    const size_t tot = (size_t)rows_2n * d;
    std::vector<uint8_t> u(tot);
    for (size_t i = 0; i < tot; ++i) {
        const double v = a[i];
        if (!(v >= 0.0 && v <= 255.0) || v != floor(v)) {
            c->err = "raw2iq: input is not byte-valued (only uint8-valued captures are supported)";
            return GSMCAL_E_UNSUPPORTED;
        }
        u[i] = (uint8_t)v;
    }
    return gsmcal_raw2iq_u8(c, u.data(), rows_2n, d, b);
}

// ---- a2 filters ----------------------------------------------------------------------------------
int gsmcal_filter(gsmcal_ctx* c, const double* coef, int ntaps, const double* s, long n, int d, int decim, double* r) {
    if (!c || !coef || !s || !r || ntaps < 1 || n < 1 || d < 1 || decim < 1) return GSMCAL_E_ARG;
    ENTER(c);
    const long nd = (n + decim - 1) / decim;
    RET_IF(upload_cached(c, c->coef, c->h_coef, coef, ntaps));
    RET_IF(upload_array(c, s, (size_t)n * d));
    RET_IF(ensure(c, c->arr_out, (size_t)nd * d * sizeof(cplx)));
    LAUNCH(c, k_fir_arr, dim3((unsigned)((nd + 255) / 256), d), dim3(256), 0, (const cplx*)c->arr_in.p, n, n,
           (const double*)c->coef.p, ntaps, decim, nd, (cplx*)c->arr_out.p, nd);
    CHECK_LAUNCH(c);
    HIPCHK(c, hipMemcpyAsync(r, c->arr_out.p, (size_t)nd * d * sizeof(cplx), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int gsmcal_chn_filter_8x_4x(gsmcal_ctx* c, const double* s, long n, int d, const double* num, int ntaps, double* r) {
    if (!num || ntaps <= 0) { num = GSM_CHN_FILTER_8X_NUM; ntaps = 60; }
    return gsmcal_filter(c, num, ntaps, s, n, d, 2, r);   // chn_filter_8x_4x.m:13,15
}

int gsmcal_chn_filter_4x(gsmcal_ctx* c, const double* s, long n, int d, const double* num, int ntaps, double* r) {
    if (!num || ntaps <= 0) { num = GSM_CHN_FILTER_4X_NUM; ntaps = 30; }
    return gsmcal_filter(c, num, ntaps, s, n, d, 1, r);   // chn_filter_4x.m:13: no decimation
}

// ---- a3..a5 coarse detector -----------------------------------------------------------------------
static int coarse_api(gsmcal_ctx* c, const double* s, long len, CoarseArgs a, StreamState* out) {
    ENTER(c);
    int fft_len = a.fft_len;
    long n_first = len;
    if (a.mode == 0) {
        // (above 74 the windows would be shorter than two samples -- refused below; above 148 the exponent would be negative)
        fft_len = a.decimation_ratio > 74 ? 0 : 1 << (int)floor(log2(148.0 / (double)a.decimation_ratio));
        n_first = (long)ceil(23.0 * 1250.0 / (double)a.decimation_ratio);
    }
    if (fft_len < 2 || fft_len > 64) return GSMCAL_E_UNSUPPORTED;
    const long nwin = n_first - (fft_len - 1);
    const size_t lds = cs_carve(false, n_first > 0 ? n_first : 0, a.mode == 0 ? 10 * fft_len : a.mv_len).launch;
    if (lds > 159 * 1024) return GSMCAL_E_UNSUPPORTED;
    // (the refusals above are decided before anything is uploaded)
    RET_IF(upload_array(c, s, (size_t)len));
    std::vector<StreamState> v(1);
    host_init_state(v[0], len);
    RET_IF(push_states(c, v));
    c->last_S = 1; c->cur = &c->lanes[0]; c->lanes[0].lo = 0; c->lanes[0].n = 1; c->n_lanes_used = 1;
    a.s = (const cplx*)c->arr_in.p; a.s_stride = len; a.len = len;
    a.th0 = c->params.coarse_th_db; a.min_hits = c->params.min_hits;
    if (a.mode != 2 && nwin >= 1 && n_first <= len) {
        RET_IF(ensure(c, c->cur->snrbuf, (size_t)nwin * sizeof(double)));
        a.snr_g = (double*)c->cur->snrbuf.p; a.snr_stride = nwin;
        if (fft_len == 16) LAUNCH(c, k_coarse_snr<true>, dim3((unsigned)((nwin + 255) / 256), 1), dim3(256), 0, a);
        else LAUNCH(c, k_coarse_snr<false>, dim3((unsigned)((nwin + 255) / 256), 1), dim3(256), 0, a);
    }
    if (fft_len == 16) LAUNCH(c, k_coarse_scan_lat, dim3(1), dim3(256), lds, (StreamState*)c->cur->state.p, a);
    else LAUNCH(c, k_coarse_scan_gen, dim3(1), dim3(256), lds, (StreamState*)c->cur->state.p, a);
    CHECK_LAUNCH(c);
    RET_IF(fetch_states(c, 1, v));
    *out = v[0];
    return 0;
}

int gsmcal_move_fft_snr_runtime_avg(gsmcal_ctx* c, const double* s, long len, int mv_len, int fft_len, double th,
                                    int* hit_flag, double* hit_idx, double* hit_avg_snr, double* hit_snr) {
    if (!c || !s || len < 1 || mv_len < 1 || fft_len < 2) return GSMCAL_E_ARG;
    CoarseArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = 1; a.mv_len = mv_len; a.fft_len = fft_len; a.th = th; a.decimation_ratio = 8;
    StreamState st;
    RET_IF(coarse_api(c, s, len, a, &st));
    if (st.status < 0) return st.status;
    if (hit_flag) *hit_flag = st.coarse_hit_flag;
    if (hit_idx) *hit_idx = st.coarse_hit_flag ? st.mv_hit_idx : -1.0;
    if (hit_avg_snr) *hit_avg_snr = st.coarse_hit_flag ? st.hit_avg_snr : INFINITY;
    if (hit_snr) *hit_snr = st.coarse_hit_flag ? st.mv_hit_snr : INFINITY;
    return 0;
}

int gsmcal_specific_fft_snr_fix_avg(gsmcal_ctx* c, const double* s, long len, const double target_set[2], int fft_len,
                                    double th, double avg_snr, int* hit_flag, double* hit_idx, double* hit_snr) {
    if (!c || !s || !target_set || len < 1 || fft_len < 2) return GSMCAL_E_ARG;
    CoarseArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = 2; a.fft_len = fft_len; a.th = th; a.avg_snr = avg_snr; a.decimation_ratio = 8; a.mv_len = 1;
    a.t_lo = (long)target_set[0]; a.t_hi = (long)target_set[1];
    StreamState st;
    RET_IF(coarse_api(c, s, len, a, &st));
    if (st.status < 0) return st.status;
    if (hit_flag) *hit_flag = st.coarse_hit_flag;
    if (hit_idx) *hit_idx = st.coarse_hit_flag ? st.mv_hit_idx : -1.0;
    if (hit_snr) *hit_snr = st.coarse_hit_flag ? st.mv_hit_snr : INFINITY;
    return 0;
}

int gsmcal_FCCH_coarse_position(gsmcal_ctx* c, const double* s, long len, int decimation_ratio, double* position,
                                double* snr, int cap, int* count) {
    if (!c || !s || !position || !snr || !count || len < 1 || decimation_ratio < 1 || cap < 1) return GSMCAL_E_ARG;
    if (hits_capacity(len, decimation_ratio) > MAXH) return GSMCAL_E_CAPACITY;
    CoarseArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = 0; a.decimation_ratio = decimation_ratio;
    StreamState st;
    c->report.clear();
    RET_IF(coarse_api(c, s, len, a, &st));
    if (st.status < 0) return st.status;
    c->report = report_coarse(st);
    if (st.n_coarse == 0) {
        position[0] = -1.0; snr[0] = -1.0; *count = 1;
        return GSMCAL_S_NO_FCCH;
    }
    if (st.n_coarse > cap) return GSMCAL_E_CAPACITY;
    for (int i = 0; i < st.n_coarse; ++i) { position[i] = st.coarse_pos[i]; snr[i] = st.coarse_snr[i]; }
    *count = st.n_coarse;
    return 0;
}

// ---- a6 FCCH_fine_correction ------------------------------------------------------------------------
int gsmcal_FCCH_fine_correction(gsmcal_ctx* c, const double* s, long len, const double* base_position, int num_base,
                                int ov, double carrier_freq, double* fcch_pos, int cap_pos, int* num_pos, double* r,
                                long cap_r, long* len_r, double* sampling_ppm, double* carrier_ppm) {
    if (!c || !s || !base_position || !fcch_pos || !num_pos || len < 1 || num_base < 0 || ov < 1 || cap_pos < 1)
        return GSMCAL_E_ARG;
    if (num_base > MAXH) return GSMCAL_E_CAPACITY;
    RET_IF(api_chain_check(ov, 0));
    ENTER(c);
    const Geom g(ov);
    RET_IF(upload_array(c, s, (size_t)len));
    RET_IF(upload_cached(c, c->cf, c->h_cf, &carrier_freq, 1));
    std::vector<StreamState> v(1);
    host_init_state(v[0], len);
    v[0].n_coarse = num_base;
    for (int i = 0; i < num_base; ++i) v[0].coarse_pos[i] = base_position[i];
    RET_IF(push_states(c, v));
    c->last_S = 1; c->cur = &c->lanes[0]; c->lanes[0].lo = 0; c->lanes[0].n = 1; c->n_lanes_used = 1;
    Source src{SRC_ARR, nullptr, 0, (const cplx*)c->arr_in.p, len, nullptr, 0};
    const int H = num_base > 0 ? num_base : 1;
    c->report.clear();
    RET_IF(run_fine(c, 1, src, 0, g, H, false, -1, 0));
    RET_IF(fetch_states(c, 1, v));
    const StreamState& st = v[0];
    if (st.status < 0) return st.status;
    c->report = report_fine(st, ov, c->params.fine_max_ppm, c->params.fine_gate_snr_db);
    if (sampling_ppm) *sampling_ppm = st.sampling_ppm1;
    if (carrier_ppm) *carrier_ppm = st.carrier_ppm1;
    if (st.fcch_is_sentinel) {
        fcch_pos[0] = -1.0;
        *num_pos = 1;
    } else {
        if (st.n_fcch > cap_pos) return GSMCAL_E_CAPACITY;
        for (int i = 0; i < st.n_fcch; ++i) fcch_pos[i] = st.fcch_pos[i];
        *num_pos = st.n_fcch;
    }
    long lr = -1;
    int level = 0;
    if (st.r1_kind == 1) { lr = len; level = 0; }
    else if (st.r1_kind == 2) { lr = st.op[1].n; level = 1; }
    else if (st.r1_kind == 3) { lr = st.op[2].n; level = 2; }
    if (len_r) *len_r = lr;
    if (r && lr > 0) {
        if (lr > cap_r) return GSMCAL_E_CAPACITY;
        if (level == 0) memcpy(r, s, (size_t)lr * sizeof(cplx));
        else RET_IF(materialise_to_host(c, src, level, lr, r));
    }
    return positive_status(st, 0);
}

// ---- a7 SCH_corr_rate_correction ----------------------------------------------------------------------
int gsmcal_SCH_corr_rate_correction(gsmcal_ctx* c, const double* s, long len, const double* fcch_pos, int num_fcch,
                                    const double* sch_ts, int len_ts, int ov, double* pos_info, int cap_rows,
                                    int* num_rows, double* r, long cap_r, long* len_r, double* sampling_ppm) {
    if (!c || !fcch_pos || !sch_ts || !pos_info || !num_rows || num_fcch < 0 || len_ts < 1 || ov < 1 || cap_rows < 1)
        return GSMCAL_E_ARG;
    if (num_fcch > MAXH) return GSMCAL_E_CAPACITY;
    RET_IF(api_chain_check(ov, len_ts));
    ENTER(c);
    const Geom g(ov);
    const bool have_s = s != nullptr && len >= 1;   // r = -1 from a failed fine stage arrives as s = NULL
    if (have_s) RET_IF(upload_array(c, s, (size_t)len));
    RET_IF(upload_cached(c, c->ts, c->h_ts, sch_ts, (size_t)2 * len_ts));
    std::vector<StreamState> v(1);
    host_init_state(v[0], have_s ? len : 0);
    const bool sentinel_in = (num_fcch == 1 && fcch_pos[0] == -1.0);
    v[0].fcch_is_sentinel = sentinel_in ? 1 : 0;
    v[0].n_fcch = sentinel_in ? 0 : num_fcch;
    for (int i = 0; i < num_fcch; ++i) v[0].fcch_pos[i] = fcch_pos[i];
    if (!have_s && !(sentinel_in || num_fcch < 5)) return GSMCAL_E_ARG;
    RET_IF(push_states(c, v));
    c->last_S = 1; c->cur = &c->lanes[0]; c->lanes[0].lo = 0; c->lanes[0].n = 1; c->n_lanes_used = 1;
    Source src{SRC_ARR, nullptr, 0, (const cplx*)c->arr_in.p, len, nullptr, 0};
    const int H = num_fcch > 0 ? num_fcch : 1;
    c->report.clear();
    RET_IF(run_sch(c, 1, src, 0, g, H, len_ts, false, -1));
    RET_IF(fetch_states(c, 1, v));
    const StreamState& st = v[0];
    if (st.status < 0) return st.status;
    c->report = report_sch(st, ov, c->params.sch_max_ppm);
    if (sampling_ppm) *sampling_ppm = st.sampling_ppm2;
    if (st.n_rows == 0) {
        // the reference's all -1 sentinel keeps the shape of the exit taken: [-1 -1] (:9, :61) or the -ones(3K,2)
        // pre-allocation of :32 (fewer than 5 SCH :84, spacing failure :106-112) -- gsm_sync_demod.m:130 counts its rows
        const int nr = st.n_sent_rows > 0 ? st.n_sent_rows : 1;
        if (nr > cap_rows) return GSMCAL_E_CAPACITY;
        for (int i = 0; i < nr; ++i) { pos_info[i] = -1.0; pos_info[cap_rows + i] = -1.0; }
        *num_rows = nr;
    } else {
        if (st.n_rows > cap_rows) return GSMCAL_E_CAPACITY;
        for (int i = 0; i < st.n_rows; ++i) {
            pos_info[i] = st.pos_info[i];
            pos_info[cap_rows + i] = st.pos_info[MAXROWS + i];
        }
        *num_rows = st.n_rows;
    }
    long lr = -1;
    int level = 0;
    if (st.r2_kind == 1) { lr = len; level = 0; }
    else if (st.r2_kind == 2) { lr = st.op[1].n; level = st.op[1].type == OP_COPY ? 0 : 1; }
    if (len_r) *len_r = lr;
    if (r && lr > 0) {
        if (lr > cap_r) return GSMCAL_E_CAPACITY;
        if (level == 0) memcpy(r, s, (size_t)lr * sizeof(cplx));
        else RET_IF(materialise_to_host(c, src, level, lr, r));
    }
    return positive_status(st, 1);
}

// ---- pos_info as the MATLAB-signature entry points get it: rows x 2, column-major, leading dimension ld --------------
// `if pos_info == -1` is true only if every element is -1
static bool pos_info_all_m1(const double* pos_info, int rows, int ld) {
    for (int i = 0; i < rows; ++i)
        if (pos_info[i] != -1.0 || pos_info[ld + i] != -1.0) return false;
    return true;
}
static int pos_info_count(const double* pos_info, int rows, int ld, double type) {
    int n = 0;
    for (int i = 0; i < rows; ++i) n += pos_info[ld + i] == type;
    return n;
}
// the table as gsmcal_calibrate_batch hands it on: [2][MAXROWS] with -1 padding (rows <= MAXROWS is the caller's check)
static std::vector<double> pos_info_padded(const double* pos_info, int rows, int ld) {
    std::vector<double> pi((size_t)2 * MAXROWS, -1.0);
    for (int i = 0; i < rows; ++i) { pi[i] = pos_info[i]; pi[MAXROWS + i] = pos_info[ld + i]; }
    return pi;
}

// ---- a8 carrier_correct_post_SCH -------------------------------------------------------------------------
int gsmcal_carrier_correct_post_SCH(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld,
                                    int ov, double carrier_freq, double* r, long cap_r, long* len_r, double* carrier_ppm) {
    if (!c || !pos_info || rows < 1 || ld < rows || ov < 1) return GSMCAL_E_ARG;
    RET_IF(api_chain_check(ov, 0));
    ENTER(c);
    const Geom g(ov);
    const bool all_m1 = pos_info_all_m1(pos_info, rows, ld);
    if (!all_m1 && rows > MAXROWS) return GSMCAL_E_CAPACITY;
    const bool have_s = s != nullptr && len >= 1;
    if (have_s) RET_IF(upload_array(c, s, (size_t)len));
    RET_IF(upload_cached(c, c->cf, c->h_cf, &carrier_freq, 1));
    std::vector<StreamState> v(1);
    host_init_state(v[0], have_s ? len : 0);
    int nfcch = 0;
    if (!all_m1) {
        v[0].n_rows = rows;
        for (int i = 0; i < rows; ++i) {
            v[0].pos_info[i] = pos_info[i];
            v[0].pos_info[MAXROWS + i] = pos_info[ld + i];
            nfcch += pos_info[ld + i] == 0.0;
        }
        if (!have_s) return GSMCAL_E_ARG;
    }
    if (nfcch > MAXH) return GSMCAL_E_CAPACITY;
    RET_IF(push_states(c, v));
    c->last_S = 1; c->cur = &c->lanes[0]; c->lanes[0].lo = 0; c->lanes[0].n = 1; c->n_lanes_used = 1;
    Source src{SRC_ARR, nullptr, 0, (const cplx*)c->arr_in.p, len, nullptr, 0};
    c->report.clear();
    RET_IF(run_post(c, 1, src, 0, g, nfcch > 0 ? nfcch : 1, false, nullptr, nullptr, nullptr));
    RET_IF(fetch_states(c, 1, v));
    const StreamState& st = v[0];
    if (st.status < 0) return st.status;
    c->report = report_post(st);
    if (carrier_ppm) *carrier_ppm = st.carrier_ppm2;
    long lr = st.r3_kind == 3 ? st.op[1].n : -1;
    if (len_r) *len_r = lr;
    if (r && lr > 0) {
        if (lr > cap_r) return GSMCAL_E_CAPACITY;
        RET_IF(materialise_to_host(c, src, 1, lr, r));
    }
    return positive_status(st, 2);
}

// ---- f4 SCH demodulator front end -------------------------------------------------------------------------
int gsmcal_SCH_equalise(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld, const double* sch_ts,
                        int len_ts, int ov, double* x_eq, int cap_bursts, int* num_bursts, int* len_fde_ov) {
    if (!c || !pos_info || !sch_ts || !num_bursts || rows < 1 || ld < rows || ov < 1 || len_ts < 1 || cap_bursts < 0) return GSMCAL_E_ARG;
    ENTER(c);
    const int L = (148 + 2 * 8 + 30) * ov, N2 = L / DM_N1;      // SCH_demod.m:22,45,53-55: round(156.25 - 8.25) + 2*8 + 30 symbols
    const int sp_t0 = (8 + 42) * ov;                            // :56 sp_of_training (0-based)
    *num_bursts = 0;
    if (len_fde_ov) *len_fde_ov = L;
    if (pos_info_all_m1(pos_info, rows, ld)) return GSMCAL_S_POST_NO_POS;      // :8
    if (!s || len < 1 || !x_eq) return GSMCAL_E_ARG;
    if (sp_t0 + len_ts > L) return GSMCAL_E_ARG;                // the training sequence must fit the window (:58)
    std::vector<long> starts;
    for (int i = 0; i < rows; ++i)
        if (pos_info[ld + i] == 1.0) starts.push_back((long)pos_info[i] - 8L * ov - 1);   // :13-14, :79 (0-based)
    const int nb = (int)starts.size();
    if (nb == 0) return 0;
    if (nb > cap_bursts) return GSMCAL_E_CAPACITY;
    const size_t lds = dm_lds_bytes(L, N2);
    if (lds > 159 * 1024) return GSMCAL_E_UNSUPPORTED;
    c->cur = &c->lanes[0];
    RET_IF(upload_array(c, s, (size_t)len));
    RET_IF(upload_cached(c, c->ts, c->h_ts, sch_ts, (size_t)2 * len_ts));
    if (c->tw_sch_n != L) {
        RET_IF(ensure(c, c->tw_sch, (size_t)L * sizeof(cplx)));
        LAUNCH(c, k_make_twiddles, dim3((L + 255) / 256), dim3(256), 0, (cplx*)c->tw_sch.p, L);
        c->tw_sch_n = L;
    }
    RET_IF(ensure(c, c->misc, (size_t)nb * (sizeof(long) + sizeof(int)) + (size_t)L * sizeof(cplx) + 64));
    cplx* d_ft = (cplx*)c->misc.p;
    long* d_start = (long*)(d_ft + L);
    int* d_status = (int*)(d_start + nb);
    RET_IF(ensure(c, c->arr_out, (size_t)nb * L * sizeof(cplx)));
    HIPCHK(c, hipMemcpyAsync(d_start, starts.data(), (size_t)nb * sizeof(long), hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, k_sch_fd_training, dim3(1), dim3(DM_THREADS), lds, (const cplx*)c->ts.p, len_ts, sp_t0, L, N2, (const cplx*)c->tw_sch.p, d_ft);
    LAUNCH(c, k_sch_equalise, dim3(nb), dim3(DM_THREADS), lds, (const cplx*)c->arr_in.p, len, (const long*)d_start, len_ts, sp_t0, L, N2,
           (const cplx*)c->tw_sch.p, (const cplx*)d_ft, (cplx*)c->arr_out.p, d_status);
    CHECK_LAUNCH(c);
    std::vector<int> st(nb);
    HIPCHK(c, hipMemcpyAsync(st.data(), d_status, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(x_eq, c->arr_out.p, (size_t)nb * L * sizeof(cplx), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < nb; ++i)
        if (st[i] != 0) return st[i];                           // MATLAB: index exceeds matrix dimensions at s(sp:ep), :81
    *num_bursts = nb;
    return 0;
}

// ---- the demod family: FCCH_demod, BCCH_demod, SCH_decode, BCCH_decode ------------------------------------------------
// Each takes (r, r_len, pos_info) of d streams -- r[d][stride] complex, pos_info[d][2][MAXROWS] -- and runs on the context's
// stream (ENTER_ON_CTX_STREAM).  What the entry points have in common: the argument check, the three input stages of the host
// forms and their device pointers.  (The macros read the host forms' parameter names.)
static bool post_args_ok(const gsmcal_ctx* c, const void* r, const void* r_len, const void* pos_info, const void* out, int d, long stride) {
    return c && r && r_len && pos_info && out && d >= 1 && stride >= 1;
}
#define POST_STAGES_IN                                                          \
    STAGE(fd_in, (size_t)d * stride * sizeof(cplx), r, nullptr, 0),             \
    STAGE(fd_len, (size_t)d * sizeof(long), r_len, nullptr, 0),                 \
    STAGE(fd_pos, (size_t)d * 2 * MAXROWS * sizeof(double), pos_info, nullptr, 0)
#define POST_STAGED_IN (const double*)c->fd_in.p, stride, (const long*)c->fd_len.p, (const double*)c->fd_pos.p

// ---- FCCH_demod.m:5-66: the check behind the calibration ------------------------------------------------------
// k_fcch_demod (one workgroup per burst slot and stream) + k_fcch_demod_finish (one wave per stream).
// The per-burst half, which gsmcal_bcch_demod_batch_dev runs too (BCCH_demod.m:49-68 is the same block): fd_part[d][MAXH][FD_PART]
// and the carrier frequencies in fd_cf.  The caller has checked its arguments and the oversampling ratio (fcch_demod_ov_ok).
static bool fcch_demod_ov_ok(int ov) { return ov <= 256 && fd_lds_bytes(148 * ov) <= 159 * 1024; }
static int fcch_demod_parts(gsmcal_ctx* c, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info, int d, int ov,
                     const double* carrier_freq) {
    const int nfft = 148 * ov;                                  // FCCH_demod.m:13-16
    const size_t lds = fd_lds_bytes(nfft);
    const double fs = GSM_SYMBOL_RATE * (double)ov;             // :30-31
    const int hnl = (int)ceil(((double)nfft * 200e3 / fs) / 2.0);   // :53 half_noise_len (55 for every ov)
    if (c->fd_tw_n != nfft) {
        RET_IF(ensure(c, c->fd_tw, (size_t)nfft * sizeof(cplx)));
        LAUNCH(c, k_make_twiddles, dim3((nfft + 255) / 256), dim3(256), 0, (cplx*)c->fd_tw.p, nfft);
        c->fd_tw_n = nfft;
    }
    RET_IF(upload_if_changed(c, c->fd_cf, c->h_fd_cf, carrier_freq, (size_t)d, "FCCH_demod carrier_freq"));
    RET_IF(ensure(c, c->fd_part, (size_t)d * MAXH * FD_PART * sizeof(double)));
    double* part = (double*)c->fd_part.p;
    for_capture_chunks(d, [&](long lo, int S) {
        LAUNCH(c, k_fcch_demod, dim3(MAXH, S), dim3(FD_THREADS), lds, (const cplx*)d_r + (size_t)lo * stride, stride, d_r_len + lo,
               d_pos_info + (size_t)lo * 2 * MAXROWS, nfft, ov, hnl, (const cplx*)c->fd_tw.p, part + (size_t)lo * MAXH * FD_PART);
    });
    return 0;
}

int gsmcal_fcch_demod_batch_dev(gsmcal_ctx* c, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info, int d,
                                int ov, const double* carrier_freq, double* d_out) {
    if (!post_args_ok(c, d_r, d_r_len, d_pos_info, d_out, d, stride) || !carrier_freq || ov < 1) return GSMCAL_E_ARG;
    if (!fcch_demod_ov_ok(ov)) return GSMCAL_E_UNSUPPORTED;
    ENTER_ON_CTX_STREAM(c);
    RET_IF(fcch_demod_parts(c, d_r, stride, d_r_len, d_pos_info, d, ov, carrier_freq));
    LAUNCH(c, k_fcch_demod_finish, dim3(d), dim3(64), 0, d_r_len, stride, d_pos_info, (const double*)c->fd_cf.p, (const double*)c->fd_part.p, d_out);
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_fcch_demod_batch(gsmcal_ctx* c, const double* r, long stride, const long* r_len, const double* pos_info, int d, int ov,
                            const double* carrier_freq, double* out) {
    if (!post_args_ok(c, r, r_len, pos_info, out, d, stride) || !carrier_freq || ov < 1) return GSMCAL_E_ARG;
    ENTER(c);
    const Stage io[] = {POST_STAGES_IN, STAGE(fd_out, (size_t)d * GSMCAL_DEMOD_COLS * sizeof(double), nullptr, out, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_fcch_demod_batch_dev(c, POST_STAGED_IN, d, ov, carrier_freq, (double*)c->fd_out.p));
    return stage_down(c, io);
}

int gsmcal_FCCH_demod(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld, int ov, double carrier_freq,
                      double* freq, double* snr, double* max_idx, int cap, int* num_fcch, double* mean_freq, double* carrier_ppm) {
    if (!c || !pos_info || !num_fcch || rows < 1 || ld < rows || ov < 1 || cap < 0) return GSMCAL_E_ARG;
    ENTER(c);
    *num_fcch = 0;
    if (mean_freq) *mean_freq = NAN;
    if (carrier_ppm) *carrier_ppm = NAN;
    std::vector<double> row(GSMCAL_DEMOD_COLS, NAN);
    if (pos_info_all_m1(pos_info, rows, ld)) {                  // :8
        row[GSMCAL_D_STATUS] = GSMCAL_S_POST_NO_POS;
        c->report = report_fcch_demod(row.data());
        return GSMCAL_S_POST_NO_POS;
    }
    const int nb = pos_info_count(pos_info, rows, ld, 0.0);
    if (!s || len < 1) return GSMCAL_E_ARG;
    if (rows > MAXROWS || nb > MAXH || nb > cap) return GSMCAL_E_CAPACITY;
    if (nb > 0 && (!freq || !snr || !max_idx)) return GSMCAL_E_ARG;
    RET_IF(gsmcal_fcch_demod_batch(c, s, len, &len, pos_info_padded(pos_info, rows, ld).data(), 1, ov, &carrier_freq, row.data()));
    const int status = (int)row[GSMCAL_D_STATUS];
    if (status < 0) return status;                              // MATLAB: index exceeds matrix dimensions at s(sp:ep), :26
    for (int i = 0; i < nb; ++i) { freq[i] = row[GSMCAL_D_FREQ + i]; snr[i] = row[GSMCAL_D_SNR + i]; max_idx[i] = row[GSMCAL_D_MAX_IDX + i]; }
    *num_fcch = nb;
    if (mean_freq) *mean_freq = row[GSMCAL_D_MEAN_FREQ];
    if (carrier_ppm) *carrier_ppm = row[GSMCAL_D_CARRIER_PPM];
    c->report = report_fcch_demod(row.data());
    return status;
}

// ---- BCCH_demod.m: the training sequence code of the BCCH bursts ---------------------------------------------------
// k_fcch_demod (the tone estimates of :49-68), k_bcch_corr (BC_GRID_X workgroups per stream, striding over its BCCH rows),
// k_bcch_finish (one wave per stream) and, when r is asked for, k_bcch_rotate, in FCCH_demod's workspace plus bc_*.
static int bcch_r_out_check(gsmcal_ctx* c, const double* r, long stride, int d, const double* r_out, const long* r_len_out) {
    if ((r_out != nullptr) != (r_len_out != nullptr)) { c->err = "BCCH_demod: r_out and r_len_out go together"; return GSMCAL_E_ARG; }
    if (r_out) {                                                // a stream rotated in place would be read after it was written
        const uintptr_t a = (uintptr_t)r, b = (uintptr_t)r_out, bytes = (uintptr_t)d * (uintptr_t)stride * sizeof(cplx);
        if (a < b + bytes && b < a + bytes) { c->err = "BCCH_demod: r_out overlaps r"; return GSMCAL_E_ARG; }
    }
    return 0;
}

int gsmcal_bcch_demod_batch_dev(gsmcal_ctx* c, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info, int d,
                                int ov, const double* nts, int len_ts, const double* carrier_freq, double* d_out, double* d_corr,
                                double* d_r_out, long* d_r_len_out) {
    if (!post_args_ok(c, d_r, d_r_len, d_pos_info, d_out, d, stride) || !nts || !carrier_freq || ov < 1) return GSMCAL_E_ARG;
    if (!fcch_demod_ov_ok(ov)) return GSMCAL_E_UNSUPPORTED;
    if (len_ts != 26 * ov) { c->err = "BCCH_demod: the templates must be 26*oversampling_ratio samples long"; return GSMCAL_E_ARG; }
    RET_IF(bcch_r_out_check(c, d_r, stride, d, d_r_out, d_r_len_out));
    ENTER_ON_CTX_STREAM(c);
    RET_IF(fcch_demod_parts(c, d_r, stride, d_r_len, d_pos_info, d, ov, carrier_freq));
    RET_IF(upload_if_changed(c, c->bc_ts, c->h_bc_ts, nts, (size_t)2 * 8 * len_ts, "BCCH_demod templates"));
    RET_IF(ensure(c, c->bc_corr, (size_t)d * BC_SLOTS * 8 * sizeof(cplx)));
    RET_IF(ensure(c, c->bc_flag, (size_t)d * BC_SLOTS * sizeof(int)));
    const double* part = (const double*)c->fd_part.p;
    cplx* corr = (cplx*)c->bc_corr.p;
    int* flag = (int*)c->bc_flag.p;
    for_capture_chunks(d, [&](long lo, int S) {
        LAUNCH(c, k_bcch_corr, dim3(BC_GRID_X, S), dim3(BC_THREADS), (size_t)len_ts * sizeof(cplx), (const cplx*)d_r + (size_t)lo * stride,
               stride, d_r_len + lo, d_pos_info + (size_t)lo * 2 * MAXROWS, ov, (const cplx*)c->bc_ts.p, part + (size_t)lo * MAXH * FD_PART,
               corr + (size_t)lo * BC_SLOTS * 8, flag + (size_t)lo * BC_SLOTS);
    });
    LAUNCH(c, k_bcch_finish, dim3(d), dim3(64), 0, d_r_len, stride, d_pos_info, (const double*)c->fd_cf.p, part, (const cplx*)corr,
           (const int*)flag, d_out, (cplx*)d_corr, d_r_len_out);
    if (d_r_out) {
        const int gx = (int)std::max(1L, std::min(256L, (stride + 2047) / 2048));
        for_capture_chunks(d, [&](long lo, int S) {
            LAUNCH(c, k_bcch_rotate, dim3(gx, S), dim3(256), 0, (const cplx*)d_r + (size_t)lo * stride, stride, (const long*)d_r_len_out + lo,
                   (const double*)d_out + (size_t)lo * GSMCAL_BCCH_COLS, ov, (cplx*)d_r_out + (size_t)lo * stride);
        });
    }
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_bcch_demod_batch(gsmcal_ctx* c, const double* r, long stride, const long* r_len, const double* pos_info, int d, int ov,
                            const double* nts, int len_ts, const double* carrier_freq, double* out, double* corr, double* r_out,
                            long* r_len_out) {
    if (!post_args_ok(c, r, r_len, pos_info, out, d, stride) || !nts || !carrier_freq || ov < 1) return GSMCAL_E_ARG;
    RET_IF(bcch_r_out_check(c, r, stride, d, r_out, r_len_out));
    ENTER(c);
    const size_t nr = (size_t)d * stride * sizeof(cplx);
    const Stage io[] = {POST_STAGES_IN,
                        STAGE(bc_out, (size_t)d * GSMCAL_BCCH_COLS * sizeof(double), nullptr, out, 0),
                        STAGE(bc_corr_out, corr ? (size_t)d * BC_SLOTS * 8 * sizeof(cplx) : 0, nullptr, corr, 0),
                        STAGE(bc_r, r_out ? nr : 0, nullptr, r_out, 0),
                        STAGE(bc_rlen, r_out ? (size_t)d * sizeof(long) : 0, nullptr, r_len_out, 0)};
    RET_IF(stage_up(c, io));
    if (r_out) HIPCHK(c, hipMemsetAsync(c->bc_r.p, 0, nr, c->stream));      // rows the reference leaves at r = -1 come back as zeros
    RET_IF(gsmcal_bcch_demod_batch_dev(c, POST_STAGED_IN, d, ov, nts, len_ts, carrier_freq, (double*)c->bc_out.p,
                                       corr ? (double*)c->bc_corr_out.p : nullptr,
                                       r_out ? (double*)c->bc_r.p : nullptr, r_out ? (long*)c->bc_rlen.p : nullptr));
    return stage_down(c, io);
}

int gsmcal_BCCH_demod(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld, const double* nts, int len_ts,
                      int ov, double carrier_freq, int* idx, double* r, long cap_r, long* len_r, double* carrier_ppm, double* corr_val,
                      double* table_row) {
    if (!c || !pos_info || !nts || !idx || rows < 1 || ld < rows || ov < 1 || (r && !len_r)) return GSMCAL_E_ARG;
    ENTER(c);
    *idx = -1;                                                  // :6-8
    if (len_r) *len_r = -1;
    if (carrier_ppm) *carrier_ppm = -1.0;
    std::vector<double> row(GSMCAL_BCCH_COLS, NAN);
    const int n0 = pos_info_count(pos_info, rows, ld, 0.0);
    if (pos_info_all_m1(pos_info, rows, ld)) {                  // :9
        row[GSMCAL_B_NUM_BCCH] = 0.0; row[GSMCAL_B_TSC_IDX] = -1.0; row[GSMCAL_B_STATUS] = GSMCAL_S_POST_NO_POS;
        if (table_row) memcpy(table_row, row.data(), row.size() * sizeof(double));
        c->report.clear();                                      // the .m file prints nothing at :9
        return GSMCAL_S_POST_NO_POS;
    }
    if (!s || len < 1) return GSMCAL_E_ARG;
    if (rows > MAXROWS) return GSMCAL_E_CAPACITY;
    if (r && cap_r < len) return GSMCAL_E_CAPACITY;
    std::vector<double> corr((size_t)BC_SLOTS * 8 * 2);
    long lr = -1;
    RET_IF(gsmcal_bcch_demod_batch(c, s, len, &len, pos_info_padded(pos_info, rows, ld).data(), 1, ov, nts, len_ts, &carrier_freq, row.data(), corr.data(), r,
                                   r ? &lr : nullptr));
    if (table_row) memcpy(table_row, row.data(), row.size() * sizeof(double));
    const int status = (int)row[GSMCAL_B_STATUS];
    if (status < 0) return status;                              // MATLAB: index exceeds matrix dimensions at :59 or :95
    if (status == GSMCAL_S_POST_FEW_BCCH) {
        c->report = report_bcch_demod(row.data(), nullptr, 0);
        return status;
    }
    std::vector<double> fo((size_t)MAXH * FD_PART, 0.0);        // the per-burst frequencies :69 prints: stream 0 of the workspace
    if (n0 > 0) {
        HIPCHK(c, hipMemcpyAsync(fo.data(), c->fd_part.p, (size_t)n0 * FD_PART * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < n0; ++i) fo[i] = fo[(size_t)i * FD_PART];
    }
    *idx = (int)row[GSMCAL_B_TSC_IDX];
    if (len_r) *len_r = r ? lr : len;
    if (carrier_ppm) *carrier_ppm = row[GSMCAL_B_CARRIER_PPM];
    if (corr_val) memcpy(corr_val, corr.data(), (size_t)4 * 8 * 2 * sizeof(double));     // :97, 8 x 4 column-major
    c->report = report_bcch_demod(row.data(), fo.data(), n0);
    return status;
}

// ---- SCH_decode: the BSIC and the frame number in the SCH bursts -----------------------------------------
// k_sch_decode (one wave per burst slot and stream) + k_sch_finish (one wave per stream), in sd_part.
static int sch_decode_args(gsmcal_ctx* c, int ov, const double* ts, int len_ts) {
    if (ov != 2 && ov != 4 && ov != 8) { c->err = "SCH_decode: oversampling ratios 2, 4 and 8 only"; return GSMCAL_E_UNSUPPORTED; }
    if (!ts || len_ts != 64 * ov) { c->err = "SCH_decode: the template must be 64*oversampling_ratio samples long"; return GSMCAL_E_ARG; }
    return 0;
}

int gsmcal_sch_decode_batch_dev(gsmcal_ctx* c, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info, int d,
                                int ov, const double* sch_ts, int len_ts, double* d_out, double* d_soft, unsigned char* d_u) {
    if (!post_args_ok(c, d_r, d_r_len, d_pos_info, d_out, d, stride)) return GSMCAL_E_ARG;
    RET_IF(sch_decode_args(c, ov, sch_ts, len_ts));
    ENTER_ON_CTX_STREAM(c);
    RET_IF(ensure(c, c->sd_part, (size_t)d * MAXH * SD_PART * sizeof(double)));
    double* part = (double*)c->sd_part.p;
    for_capture_chunks(d, [&](long lo, int S) {
        LAUNCH(c, k_sch_decode, dim3(MAXH, S), dim3(64), 0, (const cplx*)d_r + (size_t)lo * stride, stride, d_r_len + lo,
               d_pos_info + (size_t)lo * 2 * MAXROWS, ov, part + (size_t)lo * MAXH * SD_PART,
               d_soft ? d_soft + (size_t)lo * MAXH * 148 : nullptr, d_u ? d_u + (size_t)lo * MAXH * 39 : nullptr);
    });
    LAUNCH(c, k_sch_finish, dim3(d), dim3(64), 0, d_r_len, stride, d_pos_info, ov, (const double*)part, d_out);
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_sch_decode_batch(gsmcal_ctx* c, const double* r, long stride, const long* r_len, const double* pos_info, int d, int ov,
                            const double* sch_ts, int len_ts, double* out, double* soft, unsigned char* u) {
    if (!post_args_ok(c, r, r_len, pos_info, out, d, stride)) return GSMCAL_E_ARG;
    RET_IF(sch_decode_args(c, ov, sch_ts, len_ts));
    ENTER(c);
    const Stage io[] = {POST_STAGES_IN,
                        STAGE(sd_out, (size_t)d * GSMCAL_SCH_COLS * sizeof(double), nullptr, out, 0),
                        STAGE(sd_soft, soft ? (size_t)d * MAXH * 148 * sizeof(double) : 0, nullptr, soft, 0),
                        STAGE(sd_u, u ? (size_t)d * MAXH * 39 : 0, nullptr, u, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_sch_decode_batch_dev(c, POST_STAGED_IN, d, ov, sch_ts, len_ts, (double*)c->sd_out.p,
                                       soft ? (double*)c->sd_soft.p : nullptr, u ? (unsigned char*)c->sd_u.p : nullptr));
    return stage_down(c, io);
}

int gsmcal_SCH_decode(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld, const double* sch_ts,
                      int len_ts, int ov, int* bsic, long* fn_anchor, long* pos_anchor, double* table_row, double* soft,
                      unsigned char* u) {
    if (!c || !pos_info || rows < 1 || ld < rows) return GSMCAL_E_ARG;
    RET_IF(sch_decode_args(c, ov, sch_ts, len_ts));
    ENTER(c);
    if (bsic) *bsic = -1;
    if (fn_anchor) *fn_anchor = -1;
    if (pos_anchor) *pos_anchor = -1;
    c->report.clear();
    std::vector<double> row(GSMCAL_SCH_COLS, NAN);
    if (pos_info_all_m1(pos_info, rows, ld)) {                  // nothing to read: the batch form's row for such a stream
        row[GSMCAL_C_NUM_SCH] = row[GSMCAL_C_NUM_OK] = row[GSMCAL_C_NUM_CONSISTENT] = 0.0;
        row[GSMCAL_C_BSIC] = row[GSMCAL_C_FN_ANCHOR] = row[GSMCAL_C_POS_ANCHOR] = -1.0;
        row[GSMCAL_C_STATUS] = GSMCAL_S_POST_NO_POS;
        if (table_row) memcpy(table_row, row.data(), row.size() * sizeof(double));
        if (soft) std::fill(soft, soft + (size_t)MAXH * 148, NAN);
        if (u) memset(u, 255, (size_t)MAXH * 39);
        return GSMCAL_S_POST_NO_POS;
    }
    if (!s || len < 1) return GSMCAL_E_ARG;
    if (rows > MAXROWS) return GSMCAL_E_CAPACITY;
    RET_IF(gsmcal_sch_decode_batch(c, s, len, &len, pos_info_padded(pos_info, rows, ld).data(), 1, ov, sch_ts, len_ts, row.data(), soft, u));
    if (table_row) memcpy(table_row, row.data(), row.size() * sizeof(double));
    const int status = (int)row[GSMCAL_C_STATUS];
    if (status < 0) return status;
    if (status == 0) {
        if (bsic) *bsic = (int)row[GSMCAL_C_BSIC];
        if (fn_anchor) *fn_anchor = (long)row[GSMCAL_C_FN_ANCHOR];
        if (pos_anchor) *pos_anchor = (long)row[GSMCAL_C_POS_ANCHOR];
    }
    c->report = report_sch_decode(row.data());
    return status;
}

// ---- BCCH_decode: the system information in the BCCH blocks ----------------------------------------------
// k_bcch_decode (one workgroup per block slot and stream, one wave per burst) + k_bcch_decode_finish (one wave per stream), in bd_part.
static int bcch_decode_args(gsmcal_ctx* c, int ov, const int* tsc, int d) {
    if (ov != 2 && ov != 4 && ov != 8) { c->err = "BCCH_decode: oversampling ratios 2, 4 and 8 only"; return GSMCAL_E_UNSUPPORTED; }
    for (int i = 0; i < d; ++i)
        if (tsc[i] < 0 || tsc[i] > 7) { c->err = "BCCH_decode: the training sequence code must be 0..7"; return GSMCAL_E_ARG; }
    return 0;
}

int gsmcal_bcch_decode_batch_dev(gsmcal_ctx* c, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info, int d,
                                 int ov, const int* tsc, double* d_out, unsigned char* d_octets, double* d_soft) {
    if (!post_args_ok(c, d_r, d_r_len, d_pos_info, d_out, d, stride) || !tsc || !d_octets) return GSMCAL_E_ARG;
    RET_IF(bcch_decode_args(c, ov, tsc, d));
    ENTER_ON_CTX_STREAM(c);
    RET_IF(ensure(c, c->bd_part, (size_t)d * MAXH * BD_PART * sizeof(double)));
    RET_IF(upload_if_changed(c, c->bd_tsc, c->h_bd_tsc, tsc, (size_t)d, "BCCH_decode training sequence codes"));
    double* part = (double*)c->bd_part.p;
    const int* d_tsc = (const int*)c->bd_tsc.p;
    for_capture_chunks(d, [&](long lo, int S) {
        LAUNCH(c, k_bcch_decode, dim3(MAXH, S), dim3(256), 0, (const cplx*)d_r + (size_t)lo * stride, stride, d_r_len + lo,
               d_pos_info + (size_t)lo * 2 * MAXROWS, ov, d_tsc + lo, part + (size_t)lo * MAXH * BD_PART,
               d_octets + (size_t)lo * MAXH * GSMCAL_BLOCK_OCTETS, d_soft ? d_soft + (size_t)lo * MAXH * GSMCAL_BLOCK_CODED : nullptr);
    });
    LAUNCH(c, k_bcch_decode_finish, dim3(d), dim3(64), 0, d_r_len, stride, d_pos_info, (const double*)part, d_out);
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_bcch_decode_batch(gsmcal_ctx* c, const double* r, long stride, const long* r_len, const double* pos_info, int d, int ov,
                             const int* tsc, double* out, unsigned char* octets, double* soft) {
    if (!post_args_ok(c, r, r_len, pos_info, out, d, stride) || !tsc || !octets) return GSMCAL_E_ARG;
    RET_IF(bcch_decode_args(c, ov, tsc, d));
    ENTER(c);
    const Stage io[] = {POST_STAGES_IN,
                        STAGE(bd_out, (size_t)d * GSMCAL_SI_COLS * sizeof(double), nullptr, out, 0),
                        STAGE(bd_oct, (size_t)d * MAXH * GSMCAL_BLOCK_OCTETS, nullptr, octets, 0),
                        STAGE(bd_soft, soft ? (size_t)d * MAXH * GSMCAL_BLOCK_CODED * sizeof(double) : 0, nullptr, soft, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_bcch_decode_batch_dev(c, POST_STAGED_IN, d, ov, tsc, (double*)c->bd_out.p, (unsigned char*)c->bd_oct.p,
                                        soft ? (double*)c->bd_soft.p : nullptr));
    return stage_down(c, io);
}

int gsmcal_BCCH_decode(gsmcal_ctx* c, const double* s, long len, const double* pos_info, int rows, int ld, int tsc, int ov,
                       unsigned char* octets, double* table_row, double* soft, gsmcal_si_info* first) {
    if (!c || !pos_info || !octets || rows < 1 || ld < rows) return GSMCAL_E_ARG;
    RET_IF(bcch_decode_args(c, ov, &tsc, 1));
    ENTER(c);
    gsmcal_si_info si;
    gsmcal_si_fields(nullptr, &si);                             // valid = 0, every field -1
    if (first) *first = si;
    c->report.clear();
    std::vector<double> row(GSMCAL_SI_COLS, NAN);
    if (pos_info_all_m1(pos_info, rows, ld)) {                  // nothing to read: the batch form's row for such a stream
        row[GSMCAL_I_NUM_BLOCKS] = row[GSMCAL_I_NUM_OK] = 0.0;
        row[GSMCAL_I_FIRST_OK] = -1.0;
        row[GSMCAL_I_STATUS] = GSMCAL_S_POST_NO_POS;
        if (table_row) memcpy(table_row, row.data(), row.size() * sizeof(double));
        memset(octets, 0, (size_t)MAXH * GSMCAL_BLOCK_OCTETS);
        if (soft) std::fill(soft, soft + (size_t)MAXH * GSMCAL_BLOCK_CODED, NAN);
        return GSMCAL_S_POST_NO_POS;
    }
    if (!s || len < 1) return GSMCAL_E_ARG;
    if (rows > MAXROWS) return GSMCAL_E_CAPACITY;
    RET_IF(gsmcal_bcch_decode_batch(c, s, len, &len, pos_info_padded(pos_info, rows, ld).data(), 1, ov, &tsc, row.data(), octets, soft));
    if (table_row) memcpy(table_row, row.data(), row.size() * sizeof(double));
    const int status = (int)row[GSMCAL_I_STATUS];
    if (status < 0) return status;
    if (status == 0) {
        gsmcal_si_fields(octets + (size_t)((int)row[GSMCAL_I_FIRST_OK] - 1) * GSMCAL_BLOCK_OCTETS, &si);
        if (first) *first = si;
    }
    c->report = report_bcch_decode(row.data(), si);
    return status;
}

// ---- pair_coherence: delay, phase and drift between two corrected streams -------------------------------
// k_pair_xcorr (one workgroup per burst slot and pair, one wave per segment) + k_pair_finish (one wave per pair), in pc_part.
static int pair_coherence_args(gsmcal_ctx* c, int d, int ov, const int* pairs, const int* lag0, int P, int* max_lag, double min_coh) {
    if (!pairs || !lag0 || P < 1) return GSMCAL_E_ARG;
    if (ov != 2 && ov != 4 && ov != 8) { c->err = "pair_coherence: oversampling ratios 2, 4 and 8 only"; return GSMCAL_E_UNSUPPORTED; }
    if (*max_lag == 0) *max_lag = 2 * ov;
    if (*max_lag < 1 || *max_lag > 4 * ov) { c->err = "pair_coherence: max_lag must be 1 .. 4*oversampling_ratio"; return GSMCAL_E_ARG; }
    if (!(min_coh >= 0.0 && min_coh <= 1.0)) { c->err = "pair_coherence: min_coherence must be in [0, 1]"; return GSMCAL_E_ARG; }
    for (int i = 0; i < 2 * P; ++i)
        if (pairs[i] < 0 || pairs[i] >= d) { c->err = "pair_coherence: a pair names a stream outside the batch"; return GSMCAL_E_ARG; }
    return 0;
}

int gsmcal_pair_coherence_batch_dev(gsmcal_ctx* c, const double* d_r, long stride, const long* d_r_len, const double* d_pos_info, int d,
                                    int ov, const int* pairs, const int* lag0, int P, int max_lag, double min_coh, double* d_out,
                                    double* d_corr) {
    if (!post_args_ok(c, d_r, d_r_len, d_pos_info, d_out, d, stride)) return GSMCAL_E_ARG;
    RET_IF(pair_coherence_args(c, d, ov, pairs, lag0, P, &max_lag, min_coh));
    ENTER_ON_CTX_STREAM(c);
    std::vector<int> rec((size_t)3 * P);
    for (int i = 0; i < P; ++i) { rec[3 * i] = pairs[2 * i]; rec[3 * i + 1] = pairs[2 * i + 1]; rec[3 * i + 2] = lag0[i]; }
    RET_IF(upload_if_changed(c, c->pc_pairs, c->h_pc_pairs, rec.data(), rec.size(), "pair_coherence pairs"));
    RET_IF(ensure(c, c->pc_part, (size_t)P * PX_SLOTS * PX_PART * sizeof(double)));
    const int* d_pairs = (const int*)c->pc_pairs.p;
    double* part = (double*)c->pc_part.p;
    const size_t lds = px_lds_bytes(ov, max_lag), nl = (size_t)2 * max_lag + 1;
    for_capture_chunks(P, [&](long lo, int S) {
        LAUNCH(c, k_pair_xcorr, dim3(PX_SLOTS, S), dim3(PX_THREADS), lds, (const cplx*)d_r, stride, d_r_len, d_pos_info, ov, max_lag,
               d_pairs + (size_t)lo * 3, part + (size_t)lo * PX_SLOTS * PX_PART,
               d_corr ? (cplx*)d_corr + (size_t)lo * PX_SLOTS * nl * PX_K : nullptr);
    });
    LAUNCH(c, k_pair_finish, dim3(P), dim3(64), 0, d_r_len, stride, d_pos_info, ov, max_lag, min_coh, d_pairs, (const double*)part, d_out);
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_pair_coherence_batch(gsmcal_ctx* c, const double* r, long stride, const long* r_len, const double* pos_info, int d, int ov,
                                const int* pairs, const int* lag0, int P, int max_lag, double min_coh, double* out, double* corr) {
    if (!post_args_ok(c, r, r_len, pos_info, out, d, stride)) return GSMCAL_E_ARG;
    RET_IF(pair_coherence_args(c, d, ov, pairs, lag0, P, &max_lag, min_coh));
    ENTER(c);
    const Stage io[] = {POST_STAGES_IN,
                        STAGE(pc_out, (size_t)P * GSMCAL_PAIR_COLS * sizeof(double), nullptr, out, 0),
                        STAGE(pc_corr, corr ? (size_t)P * PX_SLOTS * (2 * max_lag + 1) * PX_K * sizeof(cplx) : 0, nullptr, corr, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_pair_coherence_batch_dev(c, POST_STAGED_IN, d, ov, pairs, lag0, P, max_lag, min_coh, (double*)c->pc_out.p,
                                           corr ? (double*)c->pc_corr.p : nullptr));
    return stage_down(c, io);
}

int gsmcal_pair_coherence(gsmcal_ctx* c, const double* s_a, long len_a, const double* s_b, long len_b, const double* pos_info, int rows,
                          int ld, int ov, int lag0, int max_lag, double min_coh, double* table_row, double* corr) {
    if (!c || !pos_info || !table_row || rows < 1 || ld < rows) return GSMCAL_E_ARG;
    const int pair[2] = {0, 1};
    RET_IF(pair_coherence_args(c, 2, ov, pair, &lag0, 1, &max_lag, min_coh));
    ENTER(c);
    c->report.clear();
    if (pos_info_all_m1(pos_info, rows, ld)) {                  // nothing to read: the batch form's row for such a pair
        std::fill(table_row, table_row + GSMCAL_PAIR_COLS, NAN);
        table_row[GSMCAL_P_NUM_BURSTS] = table_row[GSMCAL_P_NUM_EVAL] = table_row[GSMCAL_P_NUM_USED] = table_row[GSMCAL_P_NUM_ADJACENT] = 0.0;
        table_row[GSMCAL_P_LAG0] = (double)lag0;
        table_row[GSMCAL_P_MAX_LAG] = (double)max_lag;
        table_row[GSMCAL_P_STATUS] = GSMCAL_S_POST_NO_POS;
        if (corr) std::fill(corr, corr + (size_t)PX_SLOTS * (2 * max_lag + 1) * PX_K * 2, NAN);
        return GSMCAL_S_POST_NO_POS;
    }
    if (!s_a || !s_b || len_a < 1 || len_b < 1) return GSMCAL_E_ARG;
    if (rows > MAXROWS) return GSMCAL_E_CAPACITY;
    const long stride = std::max(len_a, len_b);                 // the two streams as one batch: a is stream 0, b stream 1 with no table
    std::vector<double> r((size_t)2 * stride * 2, 0.0);
    memcpy(r.data(), s_a, (size_t)len_a * sizeof(cplx));
    memcpy(r.data() + (size_t)stride * 2, s_b, (size_t)len_b * sizeof(cplx));
    const long r_len[2] = {len_a, len_b};
    std::vector<double> pi = pos_info_padded(pos_info, rows, ld);
    pi.resize((size_t)2 * 2 * MAXROWS, -1.0);
    RET_IF(gsmcal_pair_coherence_batch(c, r.data(), stride, r_len, pi.data(), 2, ov, pair, &lag0, 1, max_lag, min_coh, table_row, corr));
    const int status = (int)table_row[GSMCAL_P_STATUS];
    if (status < 0) return status;
    c->report = report_pair_coherence(table_row);
    return status;
}

// ---- pair_align: streams onto one dongle's time base, their carrier taken out, and their sum ------------------
// k_pair_align (one workgroup per tile of PA_TILE output samples; the members in list order when the sum is asked for, one member
// per grid row otherwise) + k_pair_align_info (one wave: the members' valid intervals and the sum's row).
static int pair_align_args(gsmcal_ctx* c, int d, int ov, const int* members, const double* params, int G, long out_len, const void* aligned,
                           const void* combined) {
    if (!members || !params || (!aligned && !combined)) return GSMCAL_E_ARG;
    if (ov != 2 && ov != 4 && ov != 8) { c->err = "pair_align: oversampling ratios 2, 4 and 8 only"; return GSMCAL_E_UNSUPPORTED; }
    if (G < 1 || G > GSMCAL_MAX_ALIGN_MEMBERS) { c->err = "pair_align: 1 .. 64 members"; return GSMCAL_E_ARG; }
    if (out_len < 1) { c->err = "pair_align: out_len must be at least 1"; return GSMCAL_E_ARG; }
    for (int g = 0; g < G; ++g) {
        if (members[g] < 0 || members[g] >= d) { c->err = "pair_align: a member names a stream outside the batch"; return GSMCAL_E_ARG; }
        if (fabs(params[(size_t)g * GSMCAL_ALIGN_PARAMS + GSMCAL_A_SLOPE_PPM]) > 1000.0) {       // (NaN passes: the member is skipped)
            c->err = "pair_align: |slope_ppm| must be at most 1000";
            return GSMCAL_E_ARG;
        }
    }
    return 0;
}

int gsmcal_pair_align_batch_dev(gsmcal_ctx* c, const double* d_r, long stride, const long* d_r_len, int d, int ov, const int* members,
                                const double* params, int G, long out_len, double* d_aligned, double* d_combined, double* d_info) {
    if (!c || !d_r || !d_r_len || !d_info || d < 1 || stride < 1) return GSMCAL_E_ARG;
    RET_IF(pair_align_args(c, d, ov, members, params, G, out_len, d_aligned, d_combined));
    ENTER_ON_CTX_STREAM(c);
    RET_IF(upload_if_changed(c, c->pa_members, c->h_pa_members, members, (size_t)G, "pair_align members"));
    RET_IF(upload_if_changed(c, c->pa_params, c->h_pa_params, params, (size_t)G * GSMCAL_ALIGN_PARAMS, "pair_align params"));
    const int* d_members = (const int*)c->pa_members.p;
    const double* d_params = (const double*)c->pa_params.p;
    const long tiles = (out_len + PA_TILE - 1) / PA_TILE, per_launch = 1L << 30;                   // (grid.x holds 2^31 - 1)
    for (long t = 0; t < tiles; t += per_launch)
        LAUNCH(c, k_pair_align, dim3((unsigned)std::min(per_launch, tiles - t), d_combined ? 1 : G), dim3(PA_TILE), 0, (const cplx*)d_r, stride,
               d_r_len, ov, d_members, d_params, G, out_len, t * PA_TILE, (cplx*)d_aligned, (cplx*)d_combined);
    LAUNCH(c, k_pair_align_info, dim3(1), dim3(64), 0, d_r_len, stride, ov, d_members, d_params, G, out_len, d_info);
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_pair_align_batch(gsmcal_ctx* c, const double* r, long stride, const long* r_len, int d, int ov, const int* members,
                            const double* params, int G, long out_len, double* aligned, double* combined, double* info) {
    if (!c || !r || !r_len || !info || d < 1 || stride < 1) return GSMCAL_E_ARG;
    RET_IF(pair_align_args(c, d, ov, members, params, G, out_len, aligned, combined));
    ENTER(c);
    c->report.clear();
    const size_t row = (size_t)out_len * sizeof(cplx);
    const Stage io[] = {STAGE(fd_in, (size_t)d * stride * sizeof(cplx), r, nullptr, 0),
                        STAGE(fd_len, (size_t)d * sizeof(long), r_len, nullptr, 0),
                        STAGE(pa_aligned, aligned ? (size_t)G * row : 0, nullptr, aligned, 0),
                        STAGE(pa_combined, combined ? row : 0, nullptr, combined, 0),
                        STAGE(pa_info, (size_t)(G + 1) * GSMCAL_ALIGN_INFO_COLS * sizeof(double), nullptr, info, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_pair_align_batch_dev(c, (const double*)c->fd_in.p, stride, (const long*)c->fd_len.p, d, ov, members, params, G, out_len,
                                       aligned ? (double*)c->pa_aligned.p : nullptr, combined ? (double*)c->pa_combined.p : nullptr,
                                       (double*)c->pa_info.p));
    RET_IF(stage_down(c, io));
    c->report = report_pair_align(members, info, G, combined != nullptr);
    return 0;
}

int gsmcal_pair_align(gsmcal_ctx* c, const double* s, long len, int ov, const double* params_row, long out_len, double* out,
                      double* info_row) {
    if (!c || !params_row || !out || !info_row || (len >= 1 && !s)) return GSMCAL_E_ARG;
    const int member = 0;
    const double none[2] = {0.0, 0.0};                           // an empty stream: one sample that is never read
    const long stride = len >= 1 ? len : 1;
    double info[2 * GSMCAL_ALIGN_INFO_COLS];
    RET_IF(gsmcal_pair_align_batch(c, len >= 1 ? s : none, stride, &len, 1, ov, &member, params_row, 1, out_len, out, nullptr, info));
    std::copy(info, info + GSMCAL_ALIGN_INFO_COLS, info_row);
    return (int)info[GSMCAL_AI_STATUS];
}

int gsmcal_pair_align_params(const double* pair_row, int ov, double min_coh, double weight, double* params_row) {
    if (!pair_row || !params_row || (ov != 2 && ov != 4 && ov != 8)) return GSMCAL_E_ARG;
    std::fill(params_row, params_row + GSMCAL_ALIGN_PARAMS, NAN);
    params_row[GSMCAL_A_WEIGHT] = weight;
    if (!(pair_row[GSMCAL_P_STATUS] == 0.0)) return GSMCAL_S_ALIGN_SKIPPED;
    int first = -1;
    for (int j = 0; j < GSMCAL_MAX_PAIR_BURSTS && first < 0; ++j)
        if (pair_row[GSMCAL_P_POS + j] == pair_row[GSMCAL_P_POS + j] && pair_row[GSMCAL_P_EDGE + j] == 0.0 &&
            pair_row[GSMCAL_P_COH + j] >= min_coh)
            first = j;
    if (first < 0) return GSMCAL_S_ALIGN_SKIPPED;
    const double p0 = round(pair_row[GSMCAL_P_POS + first]) - 1.0, half = (148.0 * ov - 1.0) / 2.0;
    const double ppm = pair_row[GSMCAL_P_REL_SAMPLING_PPM], s = 1e-6 * ppm;
    params_row[GSMCAL_A_ANCHOR] = p0 + half;
    params_row[GSMCAL_A_DELAY] = pair_row[GSMCAL_P_DELAY0] + s * half;
    params_row[GSMCAL_A_SLOPE_PPM] = ppm;
    params_row[GSMCAL_A_CARRIER_HZ] = pair_row[GSMCAL_P_REL_CARRIER_HZ] * (1.0 + s);
    params_row[GSMCAL_A_PHASE] = pair_row[GSMCAL_P_PHASE0];
    return 0;
}

// ---- optimal combining: covariance of the aligned streams, the weights, the beams ------------------------------
// k_array_cov (one workgroup per window and chunk of GSMCAL_COV_CHUNK samples) + k_array_cov_reduce (one per window: the chunk
// partials in chunk order, both triangles); k_array_combine (one workgroup per AC_TILE output samples, every beam at once).
#define AC_MAX_PARTIALS 4096L   /* chunk partials one k_array_cov launch leaves in the workspace (33 KB each at G = 64: 136 MB); a window with more is a launch of its own */

static int array_rows_args(gsmcal_ctx* c, long stride, int d, const int* rows, int G) {
    if (!rows || d < 1 || stride < 1) return GSMCAL_E_ARG;
    if (G < 1 || G > GSMCAL_MAX_ALIGN_MEMBERS) { c->err = "array: 1 .. 64 rows"; return GSMCAL_E_ARG; }
    for (int g = 0; g < G; ++g)
        if (rows[g] < 0 || rows[g] >= d) { c->err = "array: a row index outside the batch"; return GSMCAL_E_ARG; }
    return 0;
}

static int array_cov_args(gsmcal_ctx* c, long stride, int d, const int* rows, int G, const long* windows, int W) {
    RET_IF(array_rows_args(c, stride, d, rows, G));
    if (!windows) return GSMCAL_E_ARG;
    if (W < 1 || W > GSMCAL_MAX_COV_WINDOWS) { c->err = "array_covariance: 1 .. 256 windows"; return GSMCAL_E_ARG; }
    for (int w = 0; w < W; ++w) {
        const long start = windows[2 * w], len = windows[2 * w + 1];
        if (start < 0 || len < 0 || start > stride || len > stride - start) { c->err = "array_covariance: a window outside the rows"; return GSMCAL_E_ARG; }
    }
    return 0;
}

int gsmcal_array_covariance_batch_dev(gsmcal_ctx* c, const double* d_x, long stride, int d, const int* rows, int G, const long* windows, int W,
                                      double* d_cov) {
    if (!c || !d_x || !d_cov) return GSMCAL_E_ARG;
    RET_IF(array_cov_args(c, stride, d, rows, G, windows, W));
    ENTER_ON_CTX_STREAM(c);
    // {start, len, first partial} per window, the total behind them; launches of whole windows, at most AC_MAX_PARTIALS partials each
    std::vector<long> tab((size_t)(W + 1) * 3, 0);
    long total = 0, most = 1;
    std::vector<int> cut{0};                                       // the launches' first windows
    for (int w = 0, first_w = 0; w < W; ++w) {
        const long nch = (windows[2 * w + 1] + GSMCAL_COV_CHUNK - 1) / GSMCAL_COV_CHUNK;
        if (w > first_w && total + nch - tab[(size_t)first_w * 3 + 2] > AC_MAX_PARTIALS) { cut.push_back(w); first_w = w; }
        tab[(size_t)w * 3] = windows[2 * w];
        tab[(size_t)w * 3 + 1] = windows[2 * w + 1];
        tab[(size_t)w * 3 + 2] = total;
        total += nch;
        most = std::max(most, total - tab[(size_t)first_w * 3 + 2]);
    }
    tab[(size_t)W * 3 + 2] = total;
    cut.push_back(W);
    if (most > 0x7fffffffL) { c->err = "array_covariance: a window of more than 2^31 chunks"; return GSMCAL_E_ARG; }
    const int NB = (G + 3) / 4, ntri = NB * (NB + 1) / 2;
    RET_IF(upload_if_changed(c, c->ac_rows, c->h_ac_rows, rows, (size_t)G, "array rows"));
    RET_IF(upload_if_changed(c, c->ac_win, c->h_ac_win, tab.data(), tab.size(), "array_covariance windows"));
    RET_IF(ensure(c, c->ac_part, (size_t)most * ntri * AC_BLOCK_ENTRIES * sizeof(cplx)));
    const int* d_rows = (const int*)c->ac_rows.p;
    const long* d_win = (const long*)c->ac_win.p;
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
        const int w0 = cut[k], w1 = cut[k + 1];
        const long base = tab[(size_t)w0 * 3 + 2], n = tab[(size_t)w1 * 3 + 2] - base;
        if (n > 0)
            LAUNCH(c, k_array_cov, dim3((unsigned)n), dim3(AC_COV_LANES), 0, (const cplx*)d_x, stride, d_rows, G, d_win, w0, w1, base,
                   (cplx*)c->ac_part.p);
        LAUNCH(c, k_array_cov_reduce, dim3((unsigned)ntri, (unsigned)(w1 - w0)), dim3(256), 0, (const cplx*)c->ac_part.p, d_win, w0, base, G, (cplx*)d_cov);
    }
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_array_covariance_batch(gsmcal_ctx* c, const double* x, long stride, int d, const int* rows, int G, const long* windows, int W,
                                  double* cov) {
    if (!c || !x || !cov) return GSMCAL_E_ARG;
    RET_IF(array_cov_args(c, stride, d, rows, G, windows, W));
    ENTER(c);
    const Stage io[] = {STAGE(ac_x, (size_t)d * stride * sizeof(cplx), x, nullptr, 0),
                        STAGE(ac_cov, (size_t)W * G * G * sizeof(cplx), nullptr, cov, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_array_covariance_batch_dev(c, (const double*)c->ac_x.p, stride, d, rows, G, windows, W, (double*)c->ac_cov.p));
    return stage_down(c, io);
}

int gsmcal_combine_weights(const double* cov_signal, const double* cov_noise, int G, int ref, double* weights, double* info) {
    if (!cov_signal || !weights || !info || G < 1 || G > GSMCAL_MAX_ALIGN_MEMBERS || ref < 0 || ref >= G) return GSMCAL_E_ARG;
    static_assert(gsmcal_cw::CW_SINGULAR == GSMCAL_S_WEIGHTS_SINGULAR && gsmcal_cw::CW_MAX_G == GSMCAL_MAX_ALIGN_MEMBERS, "combine_weights.h and gsmcal.h disagree");
    return gsmcal_cw::combine_weights(cov_signal, cov_noise, G, ref, weights, info);
}

static int array_combine_args(gsmcal_ctx* c, long stride, int d, const int* rows, int G, const double* weights, int B, long out_len) {
    RET_IF(array_rows_args(c, stride, d, rows, G));
    if (!weights) return GSMCAL_E_ARG;
    if (B < 1 || B > GSMCAL_MAX_BEAMS) { c->err = "array_combine: 1 .. 16 beams"; return GSMCAL_E_ARG; }
    if (out_len < 1 || out_len > stride) { c->err = "array_combine: out_len must lie in 1 .. stride"; return GSMCAL_E_ARG; }
    return 0;
}

int gsmcal_array_combine_batch_dev(gsmcal_ctx* c, const double* d_x, long stride, int d, const int* rows, int G, const double* weights, int B,
                                   long out_len, double* d_out) {
    if (!c || !d_x || !d_out) return GSMCAL_E_ARG;
    RET_IF(array_combine_args(c, stride, d, rows, G, weights, B, out_len));
    ENTER_ON_CTX_STREAM(c);
    RET_IF(upload_if_changed(c, c->ac_rows, c->h_ac_rows, rows, (size_t)G, "array rows"));
    RET_IF(upload_if_changed(c, c->ac_w, c->h_ac_w, weights, (size_t)2 * B * G, "array_combine weights"));
    const int* d_rows = (const int*)c->ac_rows.p;
    const cplx* d_w = (const cplx*)c->ac_w.p;
    const long tiles = (out_len + AC_TILE - 1) / AC_TILE, per_launch = 1L << 30;                   // (grid.x holds 2^31 - 1)
    for (long t = 0; t < tiles; t += per_launch) {
        const dim3 grid((unsigned)std::min(per_launch, tiles - t));
#define AC_COMBINE(BT) LAUNCH(c, k_array_combine<BT>, grid, dim3(AC_TILE), 0, (const cplx*)d_x, stride, d_rows, G, d_w, B, out_len, t * AC_TILE, (cplx*)d_out)
        if (B == 1) AC_COMBINE(1);
        else if (B == 2) AC_COMBINE(2);
        else if (B <= 4) AC_COMBINE(4);
        else if (B <= 8) AC_COMBINE(8);
        else AC_COMBINE(16);
#undef AC_COMBINE
    }
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_array_combine_batch(gsmcal_ctx* c, const double* x, long stride, int d, const int* rows, int G, const double* weights, int B,
                               long out_len, double* out) {
    if (!c || !x || !out) return GSMCAL_E_ARG;
    RET_IF(array_combine_args(c, stride, d, rows, G, weights, B, out_len));
    ENTER(c);
    const Stage io[] = {STAGE(ac_x, (size_t)d * stride * sizeof(cplx), x, nullptr, 0),
                        STAGE(ac_out, (size_t)B * out_len * sizeof(cplx), nullptr, out, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_array_combine_batch_dev(c, (const double*)c->ac_x.p, stride, d, rows, G, weights, B, out_len, (double*)c->ac_out.p));
    return stage_down(c, io);
}

// ---- apply_calibration: raw bytes resampled and de-rotated by a calibration -------------------------------------------
// k_apply_calibration (one workgroup per tile of PA_TILE output samples and capture) + k_apply_info (one lane per capture: the valid
// interval).  The parameter rows change from call to call in the workload: every call turns them into the kernels' rows in the
// context's staging vector and uploads those on the stream -- no cache, no state a later call could see.
static_assert(gsmcal_ap::AP_PARAMS == GSMCAL_APPLY_PARAMS && gsmcal_ap::AP_SKIPPED == GSMCAL_S_ALIGN_SKIPPED && gsmcal_ap::AP_SIN_PHASE == GSMCAL_AP_SIN_PHASE &&
              gsmcal_ap::AP_DELAY == GSMCAL_AP_DELAY && gsmcal_ap::AP_SCALE == GSMCAL_AP_SCALE && gsmcal_ap::AP_GAIN == GSMCAL_AP_GAIN &&
              gsmcal_ap::T_TOTAL_SAMPLING_PPM == GSMCAL_T_TOTAL_SAMPLING_PPM && gsmcal_ap::T_TOTAL_CARRIER_PPM == GSMCAL_T_TOTAL_CARRIER_PPM &&
              gsmcal_ap::T_STATUS == GSMCAL_T_STATUS && gsmcal_ap::Q_DC_I == GSMCAL_Q_DC_I && gsmcal_ap::Q_DC_Q == GSMCAL_Q_DC_Q &&
              gsmcal_ap::Q_GAIN == GSMCAL_Q_GAIN && gsmcal_ap::Q_SIN_PHASE == GSMCAL_Q_SIN_PHASE && gsmcal_ap::Q_STATUS == GSMCAL_Q_STATUS &&
              gsmcal_ap::IQ_OK == GSMCAL_IQ_OK && GSMCAL_APPLY_INFO_COLS == GSMCAL_ALIGN_INFO_COLS, "apply_params.h and include/gsmcal.h disagree");

static int apply_args(gsmcal_ctx* c, const void* raw, int d, long n, double fs, const double* params, long out_len, long out_stride,
                      const void* out, const void* info) {
    if (!c) return GSMCAL_E_ARG;
    const char* why = nullptr;
    if (!raw || !params || !out || !info) why = "apply_calibration: no pointer may be NULL";
    else if (d < 1 || n < 1) why = "apply_calibration: d and n must be at least 1";
    else if (out_len < 1 || out_stride < out_len) why = "apply_calibration: out_len must be at least 1 and out_stride at least out_len";
    else if (!std::isfinite(fs) || !(fs > 0.0)) why = "apply_calibration: sample_rate must be finite and > 0";
    for (int i = 0; i < d && !why; ++i) {
        const double* p = params + (size_t)i * GSMCAL_APPLY_PARAMS;
        bool fin = true;
        for (int k = 0; k < GSMCAL_APPLY_PARAMS; ++k) fin = fin && std::isfinite(p[k]);
        if (!fin) continue;                                        // (the capture is skipped: GSMCAL_S_ALIGN_SKIPPED in its info row)
        if (fabs(p[GSMCAL_AP_SLOPE_PPM]) > 1000.0) why = "apply_calibration: |slope_ppm| must be at most 1000";
        else if (!(p[GSMCAL_AP_GAIN] > 0.0)) why = "apply_calibration: every gain must be > 0";
        else if (!(fabs(p[GSMCAL_AP_SIN_PHASE]) < 1.0)) why = "apply_calibration: every |sin_phase| must be below 1";
    }
    if (why) { c->err = why; return GSMCAL_E_ARG; }
    return 0;
}

// the parameter rows -> the kernels' rows, in the context's staging vector
static void apply_rows(gsmcal_ctx* c, int d, double fs, const double* params) {
    c->ap_stage.resize((size_t)d);
    for (int i = 0; i < d; ++i) {
        const double* p = params + (size_t)i * GSMCAL_APPLY_PARAMS;
        ApRow& a = c->ap_stage[(size_t)i];
        bool fin = true;
        for (int k = 0; k < GSMCAL_APPLY_PARAMS; ++k) fin = fin && std::isfinite(p[k]);
        memset(&a, 0, sizeof(a));
        if (!fin) continue;                                        // run = 0: nothing else of the row is read
        const double sp = p[GSMCAL_AP_SIN_PHASE], cph = sqrt(1.0 - sp * sp);
        a.delay = p[GSMCAL_AP_DELAY];
        a.slope = p[GSMCAL_AP_SLOPE_PPM] * 1e-6;
        a.w = 2.0 * PI_D * p[GSMCAL_AP_CARRIER_HZ] / fs;
        a.phase = p[GSMCAL_AP_PHASE];
        a.anchor = p[GSMCAL_AP_ANCHOR];
        a.scale = p[GSMCAL_AP_SCALE];
        a.dc_i = p[GSMCAL_AP_DC_I];
        a.dc_q = p[GSMCAL_AP_DC_Q];
        a.q_gain = 1.0 / (p[GSMCAL_AP_GAIN] * cph);
        a.q_skew = sp / cph;
        a.run = std::isfinite(a.w) && std::isfinite(a.q_gain) && std::isfinite(a.q_skew) ? 1.0 : 0.0;   // (a carrier_hz / sample_rate beyond fp64)
    }
}

static int apply_enqueue(gsmcal_ctx* c, const uint8_t* d_raw, int d, long n, double fs, const double* params, long out_len, long out_stride,
                         double* d_out, double* d_info) {
    c->cur = &c->lanes[0];                              // the context's stream; the lane's buffers are not touched
    apply_rows(c, d, fs, params);
    const size_t bytes = (size_t)d * sizeof(ApRow);
    RET_IF(ensure(c, c->ap_rows, bytes));
    HIPCHK(c, hipMemcpyAsync(c->ap_rows.p, c->ap_stage.data(), bytes, hipMemcpyHostToDevice, c->stream));
    const ApRow* rows = (const ApRow*)c->ap_rows.p;
    const long tiles = (out_len + PA_TILE - 1) / PA_TILE, per_launch = 1L << 30;                   // (grid.x holds 2^31 - 1)
    for_capture_chunks(d, [&](long lo, int S) {
        for (long t = 0; t < tiles; t += per_launch)
            LAUNCH(c, k_apply_calibration, dim3((unsigned)std::min(per_launch, tiles - t), S), dim3(PA_TILE), 0, d_raw + (size_t)lo * 2 * n, n,
                   rows + lo, out_len, out_stride, t * PA_TILE, (cplx*)d_out + (size_t)lo * out_stride);
    });
    LAUNCH(c, k_apply_info, dim3((unsigned)((d + 63) / 64)), dim3(64), 0, rows, d, n, out_len, d_info);
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_apply_calibration_batch_resident(gsmcal_ctx* c, const uint8_t* d_raw, int d, long n, double fs, const double* params, long out_len,
                                            long out_stride, double* d_out, double* d_info) {
    RET_IF(apply_args(c, d_raw, d, n, fs, params, out_len, out_stride, d_out, d_info));
    if ((uintptr_t)d_raw & 1) { c->err = "apply_calibration: d_raw must be 2-byte aligned"; return GSMCAL_E_ARG; }
    ENTER(c);
    return apply_enqueue(c, d_raw, d, n, fs, params, out_len, out_stride, d_out, d_info);
}

int gsmcal_apply_calibration_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, double fs, const double* params, long out_len,
                                   long out_stride, double* out, double* info) {
    RET_IF(apply_args(c, raw, d, n, fs, params, out_len, out_stride, out, info));
    ENTER(c);
    // the device rows are packed (stride out_len); a two-dimensional copy leaves the tail of every host row as it was
    const size_t row = (size_t)out_len * sizeof(cplx);
    const Stage io[] = {STAGE(stage_raw, (size_t)2 * n * d, raw, nullptr, 0),
                        STAGE(ap_out, (size_t)d * row, nullptr, nullptr, 0),
                        STAGE(ap_info, (size_t)d * GSMCAL_APPLY_INFO_COLS * sizeof(double), nullptr, info, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(apply_enqueue(c, (const uint8_t*)c->stage_raw.p, d, n, fs, params, out_len, out_len, (double*)c->ap_out.p, (double*)c->ap_info.p));
    HIPCHK(c, hipMemcpy2DAsync(out, (size_t)out_stride * sizeof(cplx), c->ap_out.p, row, row, (size_t)d, hipMemcpyDeviceToHost, c->stream));
    return stage_down(c, io);
}

int gsmcal_apply_params(const double* table_row, double tuned_freq, const double* iq_row, double delay, double phase, double scale,
                        double* params_row) {
    if (!table_row || !params_row) return GSMCAL_E_ARG;
    return gsmcal_ap::apply_params(table_row, tuned_freq, iq_row, delay, phase, scale, params_row);
}

// ---- row_coherence: delay, phase and drift between any rows on one nominal time base --------------------------------------
// k_row_xcorr (one workgroup per window and pair, one wave per segment, tiled over the segment) + k_row_finish (one wave per pair), in
// rc_part.  valid, starts and pairs go through the context's staging vector and are uploaded by every call: no cache, no state a
// later call could see.
static_assert(gsmcal_ar::R_STATUS == GSMCAL_R_STATUS && gsmcal_ar::R_DELAY0 == GSMCAL_R_DELAY0 && gsmcal_ar::R_REL_SAMPLING_PPM == GSMCAL_R_REL_SAMPLING_PPM &&
              gsmcal_ar::R_REL_CARRIER_HZ == GSMCAL_R_REL_CARRIER_HZ && gsmcal_ar::R_PHASE0 == GSMCAL_R_PHASE0 && gsmcal_ar::R_WIN_LEN == GSMCAL_R_WIN_LEN &&
              gsmcal_ar::R_SAMPLE_RATE == GSMCAL_R_SAMPLE_RATE && gsmcal_ar::R_MIN_COHERENCE == GSMCAL_R_MIN_COHERENCE &&
              gsmcal_ar::R_WINDOWS == GSMCAL_MAX_ROW_WINDOWS && gsmcal_ar::R_START == GSMCAL_R_START && gsmcal_ar::R_COH == GSMCAL_R_COH &&
              gsmcal_ar::R_EDGE == GSMCAL_R_EDGE && gsmcal_ar::AP_PARAMS == GSMCAL_APPLY_PARAMS && gsmcal_ar::AP_SCALE == GSMCAL_AP_SCALE &&
              gsmcal_ar::AP_ANCHOR == GSMCAL_AP_ANCHOR && gsmcal_ar::AR_SKIPPED == GSMCAL_S_ALIGN_SKIPPED && gsmcal_ar::AR_E_ARG == GSMCAL_E_ARG,
              "apply_refine.h and include/gsmcal.h disagree");

static int row_coherence_args(gsmcal_ctx* c, const void* x, long stride, int d, const long* valid, const int* pairs, const int* lag0, int P,
                              const long* starts, int W, int win_len, int M, double min_coh, double max_gap, double fs, const void* out) {
    if (!c) return GSMCAL_E_ARG;
    const char* why = nullptr;
    if (!x || !pairs || !lag0 || !starts || !out) why = "row_coherence: x, pairs, lag0, starts and out may not be NULL";
    else if (d < 1 || P < 1 || stride < 1) why = "row_coherence: d, P and stride must be at least 1";
    else if (W < 1 || W > GSMCAL_MAX_ROW_WINDOWS) why = "row_coherence: 1 .. GSMCAL_MAX_ROW_WINDOWS windows";
    else if (win_len < 16 || win_len > 65536) why = "row_coherence: win_len must be 16 .. 65536";
    else if (M < 1 || M > GSMCAL_MAX_ROW_LAG) why = "row_coherence: max_lag must be 1 .. GSMCAL_MAX_ROW_LAG";
    else if (!std::isfinite(fs) || !(fs > 0.0)) why = "row_coherence: sample_rate must be finite and > 0";
    else if (!(min_coh >= 0.0 && min_coh <= 1.0)) why = "row_coherence: min_coherence must be in [0, 1]";
    else if (!(max_gap >= 0.0)) why = "row_coherence: max_gap must be >= 0";
    for (int i = 0; i < 2 * P && !why; ++i)
        if (pairs[i] < 0 || pairs[i] >= d) why = "row_coherence: a pair names a row outside the batch";
    for (int i = 0; i < W && !why; ++i)
        if (starts[i] < 0 || (i > 0 && starts[i] <= starts[i - 1])) why = "row_coherence: starts must be >= 0 and strictly ascending";
    for (int i = 0; i < d && valid && !why; ++i)
        if (valid[2 * i] < 0 || valid[2 * i + 1] > stride || valid[2 * i] > valid[2 * i + 1]) why = "row_coherence: a valid interval must be 0 <= first <= end <= stride";
    if (why) { c->err = why; return GSMCAL_E_ARG; }
    return 0;
}

static int row_coherence_enqueue(gsmcal_ctx* c, const double* d_x, long stride, int d, const long* valid, const int* pairs, const int* lag0, int P,
                                 const long* starts, int W, int win_len, int M, double min_coh, double max_gap, double fs, double* d_out,
                                 double* d_corr) {
    c->cur = &c->lanes[0];                              // the context's stream; the lane's buffers are not touched
    std::vector<long>& h = c->rc_stage;
    h.resize((size_t)2 * d + W + (size_t)3 * P);
    for (int i = 0; i < d; ++i) { h[2 * i] = valid ? valid[2 * i] : 0; h[2 * i + 1] = valid ? valid[2 * i + 1] : stride; }
    for (int i = 0; i < W; ++i) h[(size_t)2 * d + i] = starts[i];
    long* hp = h.data() + (size_t)2 * d + W;
    for (int i = 0; i < P; ++i) { hp[3 * i] = pairs[2 * i]; hp[3 * i + 1] = pairs[2 * i + 1]; hp[3 * i + 2] = lag0[i]; }
    const size_t bytes = h.size() * sizeof(long);
    RET_IF(ensure(c, c->rc_in, bytes));
    RET_IF(ensure(c, c->rc_part, (size_t)P * W * PX_PART * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(c->rc_in.p, h.data(), bytes, hipMemcpyHostToDevice, c->stream));
    const long* dev = (const long*)c->rc_in.p;
    double* part = (double*)c->rc_part.p;
    const int Ls = win_len / 4, NL = 2 * M + 1, nj = (NL + 15) / 16;
    for_capture_chunks(P, [&](long lo, int S) {
        const RowIn in{dev, dev + (size_t)2 * d, dev + (size_t)2 * d + W + (size_t)3 * lo};
        double* pp = part + (size_t)lo * W * PX_PART;
        cplx* cc = d_corr ? (cplx*)d_corr + (size_t)lo * W * NL * PX_K : nullptr;
        if (nj <= 1) row_xcorr_launch<1>(c, (const cplx*)d_x, stride, in, W, S, Ls, M, pp, cc);
        else if (nj <= 2) row_xcorr_launch<2>(c, (const cplx*)d_x, stride, in, W, S, Ls, M, pp, cc);
        else if (nj <= 3) row_xcorr_launch<3>(c, (const cplx*)d_x, stride, in, W, S, Ls, M, pp, cc);
        else if (nj <= 5) row_xcorr_launch<5>(c, (const cplx*)d_x, stride, in, W, S, Ls, M, pp, cc);
        else row_xcorr_launch<RX_MAX_NJ>(c, (const cplx*)d_x, stride, in, W, S, Ls, M, pp, cc);
    });
    const RowIn in{dev, dev + (size_t)2 * d, dev + (size_t)2 * d + W};
    const RowPar par{(double)win_len, fs, min_coh, max_gap};
    LAUNCH(c, k_row_finish, dim3((unsigned)P), dim3(64), 0, in, W, Ls, M, par, (const double*)part, d_out);
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_row_coherence_batch_resident(gsmcal_ctx* c, const double* d_x, long stride, int d, const long* valid, const int* pairs, const int* lag0,
                                        int P, const long* starts, int W, int win_len, int max_lag, double min_coh, double max_gap, double fs,
                                        double* d_out, double* d_corr) {
    RET_IF(row_coherence_args(c, d_x, stride, d, valid, pairs, lag0, P, starts, W, win_len, max_lag, min_coh, max_gap, fs, d_out));
    ENTER(c);
    return row_coherence_enqueue(c, d_x, stride, d, valid, pairs, lag0, P, starts, W, win_len, max_lag, min_coh, max_gap, fs, d_out, d_corr);
}

int gsmcal_row_coherence_batch(gsmcal_ctx* c, const double* x, long stride, int d, const long* valid, const int* pairs, const int* lag0, int P,
                               const long* starts, int W, int win_len, int max_lag, double min_coh, double max_gap, double fs, double* out,
                               double* corr) {
    RET_IF(row_coherence_args(c, x, stride, d, valid, pairs, lag0, P, starts, W, win_len, max_lag, min_coh, max_gap, fs, out));
    ENTER(c);
    const Stage io[] = {STAGE(rc_x, (size_t)d * stride * sizeof(cplx), x, nullptr, 0),
                        STAGE(rc_out, (size_t)P * GSMCAL_ROW_COLS * sizeof(double), nullptr, out, 0),
                        STAGE(rc_corr, corr ? (size_t)P * W * (2 * max_lag + 1) * PX_K * sizeof(cplx) : 0, nullptr, corr, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(row_coherence_enqueue(c, (const double*)c->rc_x.p, stride, d, valid, pairs, lag0, P, starts, W, win_len, max_lag, min_coh, max_gap, fs,
                                 (double*)c->rc_out.p, corr ? (double*)c->rc_corr.p : nullptr));
    return stage_down(c, io);
}

int gsmcal_apply_params_refine(const double* coh_row, const double* params_in, double* params_out) {
    if (!coh_row || !params_in || !params_out) return GSMCAL_E_ARG;
    return gsmcal_ar::apply_params_refine(coh_row, params_in, params_out);
}

// ---- a9 total_ppm_calculation ---------------------------------------------------------------------------
int gsmcal_total_ppm_calculation(const double* ppm_in, int n, double* ppm_out) {
    if (!ppm_in || !ppm_out || n < 1) return GSMCAL_E_ARG;
    bool all_inf = true;
    for (int i = 0; i < n; ++i) all_inf = all_inf && ppm_in[i] == INFINITY;
    if (all_inf) { *ppm_out = INFINITY; return GSMCAL_S_ALL_INF; }   // :7-11
    double p = 1.0;
    for (int i = 0; i < n; ++i) p = p * (1.0 + ppm_in[i] * 1e-6);     // :14-18
    *ppm_out = (p - 1.0) * 1e6;                                        // :20-21
    return 0;
}

// ---- batched hot path ---------------------------------------------------------------------------------------
int gsmcal_frontend_batch_dev(gsmcal_ctx* c, const uint8_t* d_raw, int d, long n, const double* coef, int ntaps,
                              int decim, double* d_out) {
    if (!c || !d_raw || !coef || !d_out || d < 1 || n < 1 || ntaps < 1 || decim < 1) return GSMCAL_E_ARG;
    ENTER(c);
    c->cur = &c->lanes[0];
    c->lanes[0].lo = 0; c->lanes[0].n = d; c->n_lanes_used = 1;
    RET_IF(upload_cached(c, c->coef, c->h_coef, coef, ntaps));
    RET_IF(init_states(c, d, n));
    RET_IF(dc_means(c, d_raw, d, n));
    const long nd = (n + decim - 1) / decim;
    return fir_decim_raw(c, d_raw, d, n, (const double*)c->coef.p, ntaps, decim, (cplx*)d_out, nd);
}

int gsmcal_frontend_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, const double* coef, int ntaps, int decim,
                          double* out) {
    if (!c || !raw || !out || d < 1 || n < 1 || decim < 1) return GSMCAL_E_ARG;
    ENTER(c);
    const long nd = (n + decim - 1) / decim;
    const Stage io[] = {STAGE(misc, (size_t)2 * n * d, raw, nullptr, 0), STAGE(arr_out, (size_t)nd * d * sizeof(cplx), nullptr, out, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_frontend_batch_dev(c, (const uint8_t*)c->misc.p, d, n, coef, ntaps, decim, (double*)c->arr_out.p));
    return stage_down(c, io);
}

// ---- band power: multi_rtl_sdr_split_scanner.m:154-156, multi_rtl_sdr_diversity_scanner.m:156-158, scan_band_power_spectrum.m:80-84
// Two passes over the whole batch: k_dc_sum (exact byte sums), then k_band_power.  Cutting the batch into chunks that stay in the
// 256 MiB Infinity Cache between the passes was measured and is slower (2004 captures, 821 MB: 0.576 ms in 128 MiB chunks against
// 0.522 ms whole; profiles/band_power_chunking.json): every chunk adds two launch boundaries at which the GPU drains.
static const auto k_band_power32 = &k_band_power<32>;
static const auto k_band_power64 = &k_band_power<64>;
static const auto k_band_power128 = &k_band_power<128>;
static const auto k_band_power_any = &k_band_power<0>;

int gsmcal_band_power_batch_dev(gsmcal_ctx* c, const uint8_t* d_raw, int d, long n, const double* coef, int ntaps, int decim,
                                double* d_power) {
    if (!c || !d_raw || !coef || !d_power || d < 1 || n < 1 || n > (1L << 40) || ntaps < 1 || ntaps > BP_MAX_TAPS || decim < 1)
        return GSMCAL_E_ARG;
    ENTER(c);
    c->cur = &c->lanes[0];                              // the context's stream; the lane's buffers are not touched
    const long nd = (n + decim - 1) / decim;
    const bool sym = (ntaps == 32 || ntaps == 64 || ntaps == 128) && taps_symmetric(coef, ntaps);
    const int rows = kept_rows(decim, ntaps, (size_t)((ntaps * 8 + 15) & ~15), [&](int r) { return bp_lds_bytes(r, decim, ntaps, !sym); });
    const long nblk = (nd + rows - 1) / rows;
    if (nblk > (1L << 30)) return GSMCAL_E_ARG;
    RET_IF(upload_if_changed(c, c->bp_coef, c->h_bp_coef, coef, (size_t)ntaps, "band-power taps"));
    RET_IF(ensure(c, c->bp_state, (size_t)d * sizeof(StreamState)));
    RET_IF(ensure(c, c->bp_part, (size_t)d * nblk * sizeof(double)));
    StreamState* st = (StreamState*)c->bp_state.p;
    double* part = (double*)c->bp_part.p;
    const double* dcoef = (const double*)c->bp_coef.p;
    const size_t lds = bp_lds_bytes(rows, decim, ntaps, !sym);
    LAUNCH(c, k_band_power_clear, dim3((d + 255) / 256), dim3(256), 0, st, d);
    for_capture_chunks(d, [&](long lo, int S) {
        const uint8_t* raw = d_raw + (size_t)lo * 2 * n;
        launch_dc_sums(c, raw, S, n, st + lo);
        const dim3 grid((unsigned)nblk, S);
        const StreamState* st_lo = st + lo;
        double* part_lo = part + lo * nblk;
        if (!sym) LAUNCH(c, k_band_power_any, grid, dim3(256), lds, raw, 2 * n, st_lo, dcoef, ntaps, decim, nd, rows, part_lo);
        else if (ntaps == 32) LAUNCH(c, k_band_power32, grid, dim3(256), lds, raw, 2 * n, st_lo, dcoef, ntaps, decim, nd, rows, part_lo);
        else if (ntaps == 64) LAUNCH(c, k_band_power64, grid, dim3(256), lds, raw, 2 * n, st_lo, dcoef, ntaps, decim, nd, rows, part_lo);
        else LAUNCH(c, k_band_power128, grid, dim3(256), lds, raw, 2 * n, st_lo, dcoef, ntaps, decim, nd, rows, part_lo);
    });
    LAUNCH(c, k_band_power_finish, dim3((d + 63) / 64), dim3(64), 0, (const double*)part, (int)nblk, d, n, nd, d_power);
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_band_power_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, const double* coef, int ntaps, int decim,
                            double* power) {
    if (!c || !raw || !coef || !power || d < 1 || n < 1 || ntaps < 1 || ntaps > BP_MAX_TAPS || decim < 1) return GSMCAL_E_ARG;
    ENTER(c);
    const Stage io[] = {STAGE(stage_raw, (size_t)2 * n * d, raw, nullptr, 0), STAGE(stage_out, (size_t)d * sizeof(double), nullptr, power, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_band_power_batch_dev(c, (const uint8_t*)c->stage_raw.p, d, n, coef, ntaps, decim, (double*)c->stage_out.p));
    return stage_down(c, io);
}

// ---- sub-band power: multi_rtl_sdr_diversity_scanner_another_bak.m:186-210, every grid point inside a capture out of that capture
// The script's mixer exp(1i*(1:N)*w) is folded into the taps on the host (kernels_subband.h): one row h_k = coef_k e^{-jwk} per
// distinct finite w of the call, computed in double and cached like h_bp_coef, plus a [capture][slot] index table (-1: NaN slot).
// Passes: k_band_power_clear + k_dc_sum (exact byte sums), k_subband_power, k_subband_power_finish.
static bool sb_args_ok(const void* raw, int d, long n, const double* coef, int ntaps, int decim, const double* phase_rotate, int nsub,
                       const void* power) {
    if (!raw || !coef || !phase_rotate || !power || d < 1 || n < 1 || n > (1L << 40) || ntaps < 1 || ntaps > SB_MAX_TAPS ||
        nsub < 1 || nsub > GSMCAL_MAX_SUBBANDS || decim < 1)
        return false;
    for (size_t i = 0; i < (size_t)d * nsub; ++i)
        if (std::isinf(phase_rotate[i])) return false;
    return true;
}

int gsmcal_subband_power_batch_dev(gsmcal_ctx* c, const uint8_t* d_raw, int d, long n, const double* coef, int ntaps, int decim,
                                   const double* phase_rotate, int nsub, double* d_power) {
    if (!c || !sb_args_ok(d_raw, d, n, coef, ntaps, decim, phase_rotate, nsub, d_power)) return GSMCAL_E_ARG;
    ENTER(c);
    c->cur = &c->lanes[0];                              // the context's stream; the lane's buffers are not touched
    const long nd = (n + decim - 1) / decim;
    // kept rows per block as in gsmcal_band_power_batch_dev, with the LDS of GSMCAL_MAX_SUBBANDS tap rows set aside whatever nsub
    // is: the tiling -- and with it every bit of a sub-band's power -- depends on n, decim and ntaps only
    const int rows = kept_rows(decim, ntaps, SB_MAX_SUBBANDS * ntaps * sizeof(cplx), [&](int r) { return sb_lds_bytes(r, decim, ntaps, SB_MAX_SUBBANDS); });
    const long nblk = (nd + rows - 1) / rows;
    if (nblk > (1L << 30)) return GSMCAL_E_ARG;
    // distinct finite phases in order of first appearance (-0 counts as 0: the same taps) and the index table
    const size_t cells = (size_t)d * nsub;
    std::vector<double> w;
    std::vector<int> idx(cells);
    {
        std::unordered_map<unsigned long long, int> seen;
        for (size_t i = 0; i < cells; ++i) {
            const double v = phase_rotate[i] == 0.0 ? 0.0 : phase_rotate[i];
            if (std::isnan(v)) { idx[i] = -1; continue; }
            unsigned long long key;
            memcpy(&key, &v, sizeof(key));
            auto it = seen.find(key);
            if (it == seen.end()) { it = seen.emplace(key, (int)w.size()).first; w.push_back(v); }
            idx[i] = it->second;
        }
    }
    const bool same_coef = (int)c->h_sb_coef.size() == ntaps && memcmp(c->h_sb_coef.data(), coef, (size_t)ntaps * sizeof(double)) == 0;
    const bool same_w = c->h_sb_w.size() == w.size() && (w.empty() || memcmp(c->h_sb_w.data(), w.data(), w.size() * sizeof(double)) == 0);
    if (!w.empty() && (!same_coef || !same_w || !c->sb_taps.p)) {
        c->h_sb_coef.clear(); c->h_sb_w.clear();           // (what the rows are built from is the cache's key: set once they have gone up)
        c->h_sb_rows.resize(w.size() * ntaps * 2);
        for (size_t u = 0; u < w.size(); ++u)
            for (int m = 0; m < ntaps; ++m) {              // row[m] multiplies the sample m after the oldest: tap k = ntaps-1-m
                const int k = ntaps - 1 - m;
                c->h_sb_rows[(u * ntaps + m) * 2] = coef[k] * cos((double)k * w[u]);
                c->h_sb_rows[(u * ntaps + m) * 2 + 1] = -(coef[k] * sin((double)k * w[u]));
            }
        RET_IF(upload_host_copy(c, c->sb_taps, c->h_sb_rows, "sub-band taps"));
        c->h_sb_coef.assign(coef, coef + ntaps);
        c->h_sb_w = w;
    }
    RET_IF(upload_if_changed(c, c->sb_idx, c->h_sb_idx, idx.data(), cells, "sub-band index table"));
    RET_IF(ensure(c, c->sb_state, (size_t)d * sizeof(StreamState)));
    RET_IF(ensure(c, c->sb_part, (size_t)d * nblk * nsub * sizeof(double)));
    StreamState* st = (StreamState*)c->sb_state.p;
    double* part = (double*)c->sb_part.p;
    const int* didx = (const int*)c->sb_idx.p;
    const size_t lds = sb_lds_bytes(rows, decim, ntaps, nsub);
    LAUNCH(c, k_band_power_clear, dim3((d + 255) / 256), dim3(256), 0, st, d);
    for_capture_chunks(d, [&](long lo, int S) {
        const uint8_t* raw = d_raw + (size_t)lo * 2 * n;
        launch_dc_sums(c, raw, S, n, st + lo);
        LAUNCH(c, k_subband_power, dim3((unsigned)nblk, S), dim3(256), lds, raw, 2 * n, (const StreamState*)(st + lo),
               (const cplx*)c->sb_taps.p, didx + lo * nsub, ntaps, nsub, decim, nd, rows, part + lo * nblk * nsub);
    });
    LAUNCH(c, k_subband_power_finish, dim3((unsigned)((cells + 63) / 64)), dim3(64), 0, (const double*)part, didx, (int)nblk, d, nsub,
           n, nd, d_power);
    CHECK_LAUNCH(c);
    return 0;
}

int gsmcal_subband_power_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, const double* coef, int ntaps, int decim,
                               const double* phase_rotate, int nsub, double* power) {
    if (!c || !sb_args_ok(raw, d, n, coef, ntaps, decim, phase_rotate, nsub, power)) return GSMCAL_E_ARG;
    ENTER(c);
    const Stage io[] = {STAGE(stage_raw, (size_t)2 * n * d, raw, nullptr, 0), STAGE(stage_out, (size_t)d * nsub * sizeof(double), nullptr, power, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_subband_power_batch_dev(c, (const uint8_t*)c->stage_raw.p, d, n, coef, ntaps, decim, phase_rotate, nsub, (double*)c->stage_out.p));
    return stage_down(c, io);
}

// ---- CW sample-loss check: CW_check.m:6-8 (check_CW_samples_loss_tcp.m:70,89-90) ------------------------------------------------
// Passes (kernels_cwcheck.h): k_band_power_clear + k_dc_sum (exact byte sums), k_cw_ratio_sum, k_cw_finish_mean, k_cw_residual,
// k_cw_finish_summary.  The first pass's bytes are read again by the second: plain loads there, non-temporal ones in the second.
// `arr` != nullptr: one complex array instead of raw bytes (gsmcal_CW_check) -- the same kernels behind another load stage.
static const auto k_cw_ratio_sum_raw = &k_cw_ratio_sum<true>;
static const auto k_cw_ratio_sum_arr = &k_cw_ratio_sum<false>;
static const auto k_cw_residual_raw = &k_cw_residual<true, true>;
static const auto k_cw_residual_arr = &k_cw_residual<false, false>;
static const auto k_cw_finish_summary_raw = &k_cw_finish_summary<true>;
static const auto k_cw_finish_summary_arr = &k_cw_finish_summary<false>;
static_assert(CW_TILE == GSMCAL_CW_TILE && CW_MAX_EVENTS == GSMCAL_CW_MAX_EVENTS && CW_COLS == GSMCAL_CW_COLS && CW_ST_SHORT == GSMCAL_CW_SHORT &&
              CW_ST_ZERO == GSMCAL_CW_ZERO, "kernels_cwcheck.h and include/gsmcal.h disagree");

static int cw_enqueue(gsmcal_ctx* c, const uint8_t* d_raw, const cplx* arr, int d, long n, double thr, double* d_summary, double* d_r,
                      long r_stride) {
    c->cur = &c->lanes[0];                              // the context's stream; the lane's buffers are not touched
    const long nblk = n >= 2 ? (n - 1 + CW_TILE - 1) / CW_TILE : 0;
    if (nblk > (1L << 30)) return GSMCAL_E_ARG;
    RET_IF(ensure(c, c->cw_state, (size_t)d * sizeof(StreamState)));
    RET_IF(ensure(c, c->cw_part, (size_t)d * std::max(nblk, 1L) * sizeof(CwPart)));
    RET_IF(ensure(c, c->cw_rec, (size_t)d * std::max(nblk, 1L) * sizeof(CwRec)));
    RET_IF(ensure(c, c->cw_mean, (size_t)d * sizeof(CwMean)));
    StreamState* st = (StreamState*)c->cw_state.p;
    CwPart* part = (CwPart*)c->cw_part.p;
    CwRec* rec = (CwRec*)c->cw_rec.p;
    CwMean* mean = (CwMean*)c->cw_mean.p;
    if (nblk > 0) {
        if (!arr) LAUNCH(c, k_band_power_clear, dim3((d + 255) / 256), dim3(256), 0, st, d);
        for_capture_chunks(d, [&](long lo, int S) {
            const dim3 grid((unsigned)nblk, S);
            if (arr) {
                LAUNCH(c, k_cw_ratio_sum_arr, grid, dim3(256), 0, (const uint8_t*)nullptr, 0L, (const StreamState*)st, arr, n, n, part);
            } else {
                const uint8_t* raw = d_raw + (size_t)lo * 2 * n;
                launch_dc_sums(c, raw, S, n, st + lo);
                LAUNCH(c, k_cw_ratio_sum_raw, grid, dim3(256), 0, raw, 2 * n, (const StreamState*)(st + lo), (const cplx*)nullptr, 0L, n,
                       part + lo * nblk);
            }
        });
        LAUNCH(c, k_cw_finish_mean, dim3((d + 63) / 64), dim3(64), 0, (const CwPart*)part, (int)nblk, d, n, mean);
        for_capture_chunks(d, [&](long lo, int S) {
            const dim3 grid((unsigned)nblk, S);
            double* r_lo = d_r ? d_r + (size_t)lo * r_stride : nullptr;
            if (arr)
                LAUNCH(c, k_cw_residual_arr, grid, dim3(256), 0, (const uint8_t*)nullptr, 0L, (const StreamState*)st, arr, n, n,
                       (const CwMean*)mean, thr, r_lo, r_stride, rec);
            else
                LAUNCH(c, k_cw_residual_raw, grid, dim3(256), 0, d_raw + (size_t)lo * 2 * n, 2 * n, (const StreamState*)(st + lo),
                       (const cplx*)nullptr, 0L, n, (const CwMean*)(mean + lo), thr, r_lo, r_stride, rec + lo * nblk);
        });
    }
    if (arr)
        LAUNCH(c, k_cw_finish_summary_arr, dim3(d), dim3(256), 0, (const uint8_t*)nullptr, 0L, (const StreamState*)st, arr, n, n,
               (const CwMean*)mean, (const CwRec*)rec, (int)nblk, thr, d_summary);
    else
        LAUNCH(c, k_cw_finish_summary_raw, dim3(d), dim3(256), 0, d_raw, 2 * n, (const StreamState*)st, (const cplx*)nullptr, 0L, n,
               (const CwMean*)mean, (const CwRec*)rec, (int)nblk, thr, d_summary);
    CHECK_LAUNCH(c);
    return 0;
}

static int cw_args_ok(gsmcal_ctx* c, const void* raw, int d, long n, double thr, const void* summary, const void* r, long r_stride) {
    if (!c) return GSMCAL_E_ARG;
    const char* why = nullptr;
    if (!raw || !summary) why = "cw_check: raw and summary must not be NULL";
    else if (d < 1) why = "cw_check: d must be at least 1";
    else if (n < 1 || n > (1L << 40)) why = "cw_check: n must be 1 .. 2^40";
    else if (!(thr > 0.0) || std::isinf(thr)) why = "cw_check: thr must be finite and > 0";
    else if (r && r_stride < n - 1) why = "cw_check: r_stride is below n - 1";
    if (why) { c->err = why; return GSMCAL_E_ARG; }
    return 0;
}

int gsmcal_cw_check_batch_dev(gsmcal_ctx* c, const uint8_t* d_raw, int d, long n, double thr, double* d_summary, double* d_r,
                              long r_stride) {
    RET_IF(cw_args_ok(c, d_raw, d, n, thr, d_summary, d_r, r_stride));
    ENTER(c);
    return cw_enqueue(c, d_raw, nullptr, d, n, thr, d_summary, d_r, r_stride);
}

int gsmcal_cw_check_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, double thr, double* summary, double* r, long r_stride) {
    RET_IF(cw_args_ok(c, raw, d, n, thr, summary, r, r_stride));
    ENTER(c);
    const bool want_r = r && n >= 2;
    const Stage io[] = {STAGE(stage_raw, (size_t)2 * n * d, raw, nullptr, 0),
                        STAGE(stage_out, (size_t)d * GSMCAL_CW_COLS * sizeof(double), nullptr, summary, 0),
                        STAGE(cw_r, want_r ? (size_t)d * (n - 1) * sizeof(double) : 0, nullptr, nullptr, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(cw_enqueue(c, (const uint8_t*)c->stage_raw.p, nullptr, d, n, thr, (double*)c->stage_out.p, want_r ? (double*)c->cw_r.p : nullptr, n - 1));
    RET_IF(stage_down(c, io, false));
    if (want_r)                                         // the device rows are packed; the caller's padding is not written
        HIPCHK(c, hipMemcpy2DAsync(r, (size_t)r_stride * sizeof(double), c->cw_r.p, (size_t)(n - 1) * sizeof(double),
                                   (size_t)(n - 1) * sizeof(double), (size_t)d, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int gsmcal_CW_check(gsmcal_ctx* c, const double* s, long len, double* r, double* phase_rotate) {
    if (!c) return GSMCAL_E_ARG;
    if (!s || !r || len < 2 || len > (1L << 36)) { c->err = "CW_check: s and r must not be NULL and len must be 2 .. 2^36"; return GSMCAL_E_ARG; }
    ENTER(c);
    double row[GSMCAL_CW_COLS];
    const Stage io[] = {STAGE(cw_in, (size_t)len * sizeof(cplx), s, nullptr, 0), STAGE(stage_out, sizeof(row), nullptr, row, 0),
                        STAGE(cw_r, (size_t)(len - 1) * sizeof(double), nullptr, r, 0)};
    RET_IF(stage_up(c, io));
    // (no threshold in the MATLAB signature: one nothing exceeds, so no block is evaluated again for the event list)
    RET_IF(cw_enqueue(c, nullptr, (const cplx*)c->cw_in.p, 1, len, 1e300, (double*)c->stage_out.p, (double*)c->cw_r.p, len - 1));
    RET_IF(stage_down(c, io));
    if (phase_rotate) *phase_rotate = row[0];
    return 0;
}

// ---- I/Q imbalance and clipping check (the reference's TODO item 4.5; kernels_iqcheck.h) ---------------------------------------------
// Passes: k_iq_moments (one record per capture and tile), k_iq_finish (the whole row).  `arr` != nullptr: one complex array instead
// of raw bytes (gsmcal_IQ_imbalance).
static const auto k_iq_moments_raw = &k_iq_moments<true>;
static const auto k_iq_moments_arr = &k_iq_moments<false>;
static const auto k_iq_finish_raw = &k_iq_finish<true>;
static const auto k_iq_finish_arr = &k_iq_finish<false>;
static_assert(IQ_TILE == GSMCAL_IQ_TILE && IQ_COLS == GSMCAL_IQ_COLS && IQ_N_MAX == GSMCAL_IQ_MAX_N && IQ_ST_SHORT == GSMCAL_IQ_SHORT &&
              IQ_ST_FLAT == GSMCAL_IQ_FLAT && GSMCAL_Q_STATUS == IQ_COLS - 1, "kernels_iqcheck.h and include/gsmcal.h disagree");

static int iq_enqueue(gsmcal_ctx* c, const uint8_t* d_raw, const cplx* arr, int d, long n, double* d_table) {
    c->cur = &c->lanes[0];                              // the context's stream; the lane's buffers are not touched
    const long nblk = (n + IQ_TILE - 1) / IQ_TILE;      // n <= 2^23: at most 512
    const size_t rec = arr ? sizeof(IqPart<false>) : sizeof(IqPart<true>);
    RET_IF(ensure(c, c->iq_part, (size_t)d * nblk * rec));
    if (arr) {
        IqPart<false>* part = (IqPart<false>*)c->iq_part.p;
        LAUNCH(c, k_iq_moments_arr, dim3((unsigned)nblk, d), dim3(256), 0, (const uint8_t*)nullptr, 0L, arr, n, n, part);
        LAUNCH(c, k_iq_finish_arr, dim3((d + 3) / 4), dim3(256), 0, (const IqPart<false>*)part, (int)nblk, d, n, d_table);
    } else {
        IqPart<true>* part = (IqPart<true>*)c->iq_part.p;
        for_capture_chunks(d, [&](long lo, int S) {
            LAUNCH(c, k_iq_moments_raw, dim3((unsigned)nblk, S), dim3(256), 0, d_raw + (size_t)lo * 2 * n, 2 * n, (const cplx*)nullptr, 0L, n,
                   part + lo * nblk);
        });
        LAUNCH(c, k_iq_finish_raw, dim3((d + 3) / 4), dim3(256), 0, (const IqPart<true>*)part, (int)nblk, d, n, d_table);
    }
    CHECK_LAUNCH(c);
    return 0;
}

static int iq_args_ok(gsmcal_ctx* c, const void* raw, int d, long n, const void* table) {
    if (!c) return GSMCAL_E_ARG;
    const char* why = nullptr;
    if (!raw || !table) why = "iq_imbalance: raw and table must not be NULL";
    else if (d < 1) why = "iq_imbalance: d must be at least 1";
    else if (n < 1) why = "iq_imbalance: n must be at least 1";
    if (why) { c->err = why; return GSMCAL_E_ARG; }
    if (n > GSMCAL_IQ_MAX_N) { c->err = "iq_imbalance: n above 2^23 (the exact 64-bit moments would overflow)"; return GSMCAL_E_UNSUPPORTED; }
    return 0;
}

int gsmcal_iq_imbalance_batch_dev(gsmcal_ctx* c, const uint8_t* d_raw, int d, long n, double* d_table) {
    RET_IF(iq_args_ok(c, d_raw, d, n, d_table));
    if ((uintptr_t)d_raw & 1) { c->err = "iq_imbalance: d_raw must be 2-byte aligned"; return GSMCAL_E_ARG; }
    ENTER(c);
    return iq_enqueue(c, d_raw, nullptr, d, n, d_table);
}

int gsmcal_iq_imbalance_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, double* table) {
    RET_IF(iq_args_ok(c, raw, d, n, table));
    ENTER(c);
    const Stage io[] = {STAGE(stage_raw, (size_t)2 * n * d, raw, nullptr, 0),
                        STAGE(stage_out, (size_t)d * GSMCAL_IQ_COLS * sizeof(double), nullptr, table, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(iq_enqueue(c, (const uint8_t*)c->stage_raw.p, nullptr, d, n, (double*)c->stage_out.p));
    return stage_down(c, io);
}

int gsmcal_IQ_imbalance(gsmcal_ctx* c, const double* s, long len, double* table_row) {
    if (!c) return GSMCAL_E_ARG;
    if (!s || !table_row || len < 1) { c->err = "IQ_imbalance: s and table_row must not be NULL and len must be at least 1"; return GSMCAL_E_ARG; }
    if (len > GSMCAL_IQ_MAX_N) { c->err = "IQ_imbalance: len above 2^23"; return GSMCAL_E_UNSUPPORTED; }
    ENTER(c);
    c->report.clear();
    const Stage io[] = {STAGE(iq_in, (size_t)len * sizeof(cplx), s, nullptr, 0),
                        STAGE(stage_out, GSMCAL_IQ_COLS * sizeof(double), nullptr, table_row, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(iq_enqueue(c, nullptr, (const cplx*)c->iq_in.p, 1, len, (double*)c->stage_out.p));
    RET_IF(stage_down(c, io));
    c->report = report_iq_imbalance(table_row);
    return 0;
}

int gsmcal_iq_correct(gsmcal_ctx* c, const double* s, long len, int d, const double* gain, const double* sin_phase, double* out) {
    if (!c) return GSMCAL_E_ARG;
    const char* why = nullptr;
    if (!s || !gain || !sin_phase || !out) why = "iq_correct: no pointer may be NULL";
    else if (d < 1 || len < 1 || (size_t)d * (size_t)len > ((size_t)1 << 36)) why = "iq_correct: d and len must be at least 1 and d*len at most 2^36";
    else {
        const size_t bytes = (size_t)d * len * sizeof(cplx);
        const uintptr_t a = (uintptr_t)s, b = (uintptr_t)out;
        if (a != b && a < b + bytes && b < a + bytes) why = "iq_correct: out may equal s or lie apart from it, not overlap it";
        for (int i = 0; i < d && !why; ++i) {
            if (!std::isfinite(gain[i]) || !(gain[i] > 0.0)) why = "iq_correct: every gain must be finite and > 0";
            else if (!(fabs(sin_phase[i]) < 1.0)) why = "iq_correct: every |sin_phase| must be below 1";
        }
    }
    if (why) { c->err = why; return GSMCAL_E_ARG; }
    ENTER(c);
    c->cur = &c->lanes[0];
    std::vector<double> par((size_t)2 * d);
    for (int i = 0; i < d; ++i) { par[2 * i] = gain[i]; par[2 * i + 1] = sin_phase[i]; }
    RET_IF(upload_if_changed(c, c->iq_par, c->h_iq_par, par.data(), par.size(), "I/Q correction parameters"));
    const Stage io[] = {STAGE(iq_in, (size_t)d * len * sizeof(cplx), s, out, 0)};
    RET_IF(stage_up(c, io));
    for_capture_chunks(d, [&](long lo, int S) {
        LAUNCH(c, k_iq_correct, dim3((unsigned)((len + 1023) / 1024), S), dim3(256), 0, (cplx*)c->iq_in.p + (size_t)lo * len, len,
               (const double*)c->iq_par.p + 2 * lo);
    });
    CHECK_LAUNCH(c);
    return stage_down(c, io);
}

int gsmcal_fcch_scan_batch_dev(gsmcal_ctx* c, const uint8_t* d_raw, int d, long n, const double* coef, int ntaps,
                               double* d_snr_numhit, double* d_positions, double* d_pos_snr, int* d_counts) {
    if (!c || !d_raw || !coef || !d_snr_numhit || d < 1 || n < 1 || ntaps < 1) return GSMCAL_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int ov = 8, dec_ratio = 8, decim = ov * dec_ratio;   // ..FCCH_scanner.m:43-45
    const long nd = (n + decim - 1) / decim;
    if (hits_capacity(nd, dec_ratio) > MAXH) return GSMCAL_E_CAPACITY;
    if (nd < (long)ceil(23.0 * 1250.0 / (double)dec_ratio)) {   // FCCH_coarse_position.m:25 s(1:ceil(23 frames)): MATLAB index error
        c->err = "capture shorter than 23 frames after decimation (FCCH_coarse_position.m:25 would index past the end)";
        return GSMCAL_E_INDEX;
    }
    // Calls in flight (gsmcal_ctx_set_pipeline_depth > 1): a single-stage scanner batch (up to 1 199 captures)
    // runs on internal stream i mod depth in workspace i mod depth, so the detector of call i -- one resident round of latency-bound
    // workgroups -- sits underneath the bandwidth-bound front kernel of call i+1 (multi_rtl_sdr_gsm_FCCH_scanner.m:132-135,163-186
    // over consecutive sweeps).  Same semantics as for calibration calls: outputs complete at call i + depth / gsmcal_sync / any other
    // entry point.
    const bool pipelined = pipe_may_fly(c, d, false);
    const bool same_taps = (int)c->h_coef.size() == ntaps && memcmp(c->h_coef.data(), coef, (size_t)ntaps * sizeof(double)) == 0 && c->head_epoch == c->coef_epoch;
    if (!pipelined || !same_taps) RET_IF(pipe_join(c));
    c->cur = &c->lanes[0];
    c->detail_lane = nullptr;
    c->call_raw_bytes = (size_t)d * 2 * (size_t)n;
    c->call_raw_fresh = (const void*)d_raw != c->last_raw;
    c->last_raw = d_raw;
    RET_IF(upload_cached(c, c->coef, c->h_coef, coef, ntaps));
    RET_IF(ensure_head(c, decim));
    if (pipelined)
        return pipe_call(c, d, [&](Lane& L) -> int {
            RET_IF(ensure(c, L.dec, (size_t)d * nd * sizeof(cplx)));
            RET_IF(front_fused(c, d_raw, d, n, (const double*)c->coef.p, ntaps, decim, (cplx*)L.dec.p, nd, 0, d));
            ScanAccept acc;
            acc.snr_numhit = d_snr_numhit; acc.positions = d_positions; acc.pos_snr = d_pos_snr; acc.counts = d_counts;
            return coarse(c, d, (const cplx*)L.dec.p, nd, nd, dec_ratio, 0, true, n, decim, &acc, true);
        });
    const std::vector<uintptr_t> key = {(uintptr_t)d_raw, (uintptr_t)d, (uintptr_t)n, (uintptr_t)ntaps,
                                        (uintptr_t)d_snr_numhit, (uintptr_t)d_positions, (uintptr_t)d_pos_snr,
                                        (uintptr_t)d_counts, (uintptr_t)c->n_lanes_cfg, (uintptr_t)c->params_epoch};
    auto enqueue = [&]() -> int {
    const int nl = plan_lanes(c, d, false);
    RET_IF(fork_lanes(c, nl));
    for (int i = 0; i < nl; ++i) {
        Lane& L = c->lanes[i];
        c->cur = &L;
        const int lo = L.lo, S = L.n;
        const uint8_t* raw_i = d_raw + (size_t)lo * 2 * n;
        RET_IF(ensure(c, L.dec, (size_t)S * nd * sizeof(cplx)));
        if (nl > 1) {                                       // pipeline: this front kernel starts when the previous stage's has finished
            if (!L.front_done) HIPCHK(c, hipEventCreateWithFlags(&L.front_done, hipEventDisableTiming));
            if (i > 0) HIPCHK(c, hipStreamWaitEvent(L.stream, c->lanes[i - 1].front_done, 0));
        }
        // The next stage's front kernel waits for this one through an event, and that hand-over leaves the memory system idle for
        // ~12 us per stage (rocprofv3 timeline).  So the stage's front kernel is launched in two parts: the event sits behind the
        // first (GSMCAL_SCAN_SPLIT percent of the captures), and the rest runs on this lane underneath the start of the next stage.
        const int S_a = nl > 1 && i + 1 < nl && c->scan_split > 0 && c->scan_split < 100 ? std::max(1, (int)((long)S * c->scan_split / 100)) : S;
        RET_IF(front_fused(c, raw_i, S_a, n, (const double*)c->coef.p, ntaps, decim, (cplx*)L.dec.p, nd, 0, S));
        if (nl > 1) HIPCHK(c, hipEventRecord(L.front_done, L.stream));
        if (S_a < S) RET_IF(front_fused(c, raw_i, S - S_a, n, (const double*)c->coef.p, ntaps, decim, (cplx*)L.dec.p, nd, S_a, S));
        // the acceptance rule (multi_rtl_sdr_gsm_FCCH_scanner.m:168-185) runs at the end of k_coarse_scan, on the state it just built
        ScanAccept acc;
        acc.snr_numhit = d_snr_numhit + (size_t)2 * lo;
        acc.positions = d_positions ? d_positions + (size_t)lo * MAXH : nullptr;
        acc.pos_snr = d_pos_snr ? d_pos_snr + (size_t)lo * MAXH : nullptr;
        acc.counts = d_counts ? d_counts + lo : nullptr;
        RET_IF(coarse(c, S, (const cplx*)L.dec.p, nd, nd, dec_ratio, 0, true, n, decim, &acc, nl == 1 || S <= 3 * c->n_cu));
        CHECK_LAUNCH(c);
    }
    RET_IF(join_lanes(c, nl));
    return 0;
    };
    RET_IF(run_maybe_graph(c, pick_slot(c, c->g_scan, key), key, enqueue, plan_lanes(c, d, false) > 1));
    plan_lanes(c, d, false);
    c->cur = &c->lanes[0];
    c->last_S = d;
    return 0;
}

int gsmcal_fcch_scan_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, const double* coef, int ntaps, double* snr,
                           double* num_hit, double* positions, double* pos_snr, int* counts) {
    if (!c || !raw || !snr || !num_hit || d < 1 || n < 1) return GSMCAL_E_ARG;
    ENTER(c);
    // snrhit: [d][2] SNR and hit count | [d][MAXH] positions | [d][MAXH] their SNRs | [d] counts
    const size_t nsn = (size_t)2 * d * sizeof(double), npos = (size_t)d * MAXH * sizeof(double);
    std::vector<double> sn((size_t)2 * d);
    const Stage io[] = {STAGE(misc, (size_t)2 * n * d, raw, nullptr, 0), STAGE(snrhit, nsn + 2 * npos + (size_t)d * sizeof(int), nullptr, nullptr, 0),
                        STAGE(snrhit, nsn, nullptr, sn.data(), 0), STAGE(snrhit, npos, nullptr, positions, nsn),
                        STAGE(snrhit, npos, nullptr, pos_snr, nsn + npos), STAGE(snrhit, (size_t)d * sizeof(int), nullptr, counts, nsn + 2 * npos)};
    RET_IF(stage_up(c, io));
    double* d_sn = (double*)c->snrhit.p;
    double* d_pos = d_sn + (size_t)2 * d;
    double* d_ps = d_pos + (size_t)d * MAXH;
    int* d_cnt = (int*)(d_ps + (size_t)d * MAXH);
    RET_IF(gsmcal_fcch_scan_batch_dev(c, (const uint8_t*)c->misc.p, d, n, coef, ntaps, d_sn, d_pos, d_ps, d_cnt));
    RET_IF(pipe_join(c));                      // (a pipelined context: the copies below wait for this call like for any other)
    RET_IF(stage_down(c, io));
    for (int i = 0; i < d; ++i) { snr[i] = sn[2 * i]; num_hit[i] = sn[2 * i + 1]; }
    return 0;
}

// r_correct of the S streams of the current lane (gsm_sync_demod.m:118-120 hand it to SCH_demod): one launch on the lane's stream
static int launch_r_correct(gsmcal_ctx* c, Lane& L, const Source& src, const uint8_t* raw_i, int S, long n, int ntaps, double* d_r_correct_lane) {
    StreamTileArgs ta;
    ta.raw = raw_i; ta.raw_stride = 2 * n; ta.coef = (const double*)c->coef.p; ta.ntaps = ntaps;
    ta.dst = (cplx*)d_r_correct_lane; ta.dst_stream_stride = n;
    const size_t tlds = stream_tile_lds(ntaps);
    if (ntaps == 47 && (int)c->h_coef.size() == ntaps && taps_symmetric(c->h_coef.data(), ntaps)) {   // the drivers' filter: taps in registers, every sample read once
        LAUNCH(c, k_stream_tile_s47<ST47_TILE>, dim3((unsigned)((n + (long)ST47_TILE * ST_TPB - 1) / ((long)ST47_TILE * ST_TPB)), S), dim3(ST_THREADS), stream_tile_s47_lds(), (const StreamState*)L.state.p, ta);
        CHECK_LAUNCH(c);
    } else if (tlds <= 64 * 1024) {
        LAUNCH_GEOM(ta.ntaps == 47, c, (k_stream_tile<47>), (k_stream_tile<0>), dim3((unsigned)((n + (long)ST_TILE * ST_TPB - 1) / ((long)ST_TILE * ST_TPB)), S), dim3(ST_THREADS), tlds, (const StreamState*)L.state.p, ta);
        CHECK_LAUNCH(c);
    } else {                                        // very long filters: the general tile gather
        const int tiles = (int)((n + TILE - 1) / TILE);
        RET_IF(launch_gather(c, S, src, 4, TILE, true, tiles, (cplx*)d_r_correct_lane, n, 0));
    }
    return 0;
}

// (a call that took the fused tail: what fused_recover needs to run it again; the inputs are the context's cached copies)
static void record_fused_call(gsmcal_ctx* c, const uint8_t* d_raw, int d, long n, int ntaps, int len_ts, double* d_table, double* d_pos_info,
                              double* d_r_correct, long* d_r_len) {
    if (c->recovering) return;
    if (c->fused_calls.size() >= 16) c->fused_calls.erase(c->fused_calls.begin());      // (a caller that never synchronises through the library)
    c->fused_calls.push_back({d_raw, d, n, ntaps, len_ts, c->h_coef, c->h_ts, c->h_cf, d_table, d_pos_info, d_r_correct, d_r_len});
}

int gsmcal_calibrate_batch_dev(gsmcal_ctx* c, const uint8_t* d_raw, int d, long n, const double* coef, int ntaps,
                               const double* sch_ts, int len_ts, const double* carrier_freq, double* d_table,
                               double* d_pos_info, double* d_r_correct, long* d_r_len) {
    if (!c || !d_raw || !coef || !sch_ts || !carrier_freq || !d_table || d < 1 || n < 1 || ntaps < 1 || len_ts < 1)
        return GSMCAL_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int ov = 8, dec_ratio = 8, decim = ov * dec_ratio;   // gsm_sync_demod.m:17-19
    const Geom g(ov);
    const long nd = (n + decim - 1) / decim;
    int H = hits_capacity(nd, dec_ratio) + 1;
    if (H > MAXH) return GSMCAL_E_CAPACITY;
    // Calls in flight (gsmcal_ctx_set_pipeline_depth > 1): calls that run on one lane.  Anything that would touch what the calls in
    // flight still read (new taps / training sequence / carrier frequencies, a workspace that must grow, the twiddle table) joins
    // them into the context's stream first.
    bool want_pipe;
    const bool pipelined = pipe_may_fly(c, d, true, &want_pipe);
    // (events on every dispatch -- gsmcal_profile_enable -- or the caller's own stream capture: one call at a time, but with the
    // kernels the calls in flight run, so that a per-kernel profile of a depth-4 context describes what the depth-4 loop launches)
    const bool same_kernels_unpipelined = want_pipe && !pipelined;
    const bool same_inputs = (int)c->h_coef.size() == ntaps && memcmp(c->h_coef.data(), coef, (size_t)ntaps * sizeof(double)) == 0 &&
                             c->h_ts.size() == (size_t)2 * len_ts && memcmp(c->h_ts.data(), sch_ts, (size_t)2 * len_ts * sizeof(double)) == 0 &&
                             (int)c->h_cf.size() == d && memcmp(c->h_cf.data(), carrier_freq, (size_t)d * sizeof(double)) == 0 &&
                             c->tw_n == g.nfft && c->head_epoch == c->coef_epoch;
    if (!pipelined || !same_inputs) RET_IF(pipe_join(c));
    c->cur = &c->lanes[0];
    c->detail_lane = nullptr; c->cf_lane = nullptr;       // (also what an earlier call that failed half-way may have left set)
    c->no_fuse_now = same_kernels_unpipelined;
    c->call_raw_bytes = (size_t)d * 2 * (size_t)n;
    c->call_raw_fresh = (const void*)d_raw != c->last_raw;
    c->last_raw = d_raw;
    RET_IF(upload_cached(c, c->coef, c->h_coef, coef, ntaps));
    RET_IF(upload_cached(c, c->ts, c->h_ts, sch_ts, (size_t)2 * len_ts));
    RET_IF(upload_cached(c, c->cf, c->h_cf, carrier_freq, d));
    RET_IF(ensure_head(c, decim));
    RET_IF(ensure_twiddles(c, g.nfft));
    if (pipelined)      // front end + coarse detector (:107,110,117), fine search (:118), four-launch tail
        return pipe_call(c, d, [&](Lane& L) -> int {
            c->no_fuse_now = true;
            RET_IF(ensure(c, L.dec, (size_t)d * nd * sizeof(cplx)));
            RET_IF(front_fused(c, d_raw, d, n, (const double*)c->coef.p, ntaps, decim, (cplx*)L.dec.p, nd));
            RET_IF(coarse(c, d, (const cplx*)L.dec.p, nd, nd, dec_ratio, ov, true, n, decim));
            Source src{SRC_RAW, d_raw, 2 * n, nullptr, 0, (const double*)c->coef.p, ntaps};
            c->cf_lane = (const double*)c->cf.p;
            ChainOut co{d_table, d_pos_info, d_r_len, false};
            RET_IF(run_fine(c, d, src, 0, g, H, true, 2, len_ts, &co));
            if (!co.fused) {
                RET_IF(run_sch(c, d, src, 2, g, H, len_ts, true, 3));
                RET_IF(run_post(c, d, src, 3, g, H, true, co.table, co.pos_info_out, co.r_len_out));
            }
            return d_r_correct ? launch_r_correct(c, L, src, d_raw, d, n, ntaps, d_r_correct) : 0;
        });
    // independent streams: split over lanes (HIP streams) so latency-bound stages of one group overlap the
    // compute-bound fine search of another; a repeated call is replayed as one hipGraph
    const std::vector<uintptr_t> key = {(uintptr_t)d_raw, (uintptr_t)d, (uintptr_t)n, (uintptr_t)ntaps, (uintptr_t)len_ts,
                                        (uintptr_t)d_table, (uintptr_t)d_pos_info, (uintptr_t)d_r_correct,
                                        (uintptr_t)d_r_len, (uintptr_t)c->n_lanes_cfg, (uintptr_t)c->params_epoch};
    auto enqueue = [&]() -> int {
    const int nl = plan_lanes(c, d);
    RET_IF(fork_lanes(c, nl));
    const double* cf_all = (const double*)c->cf.p;
    for (int i = 0; i < nl; ++i) {
        Lane& L = c->lanes[i];
        c->cur = &L;
        const int lo = L.lo, S = L.n;
        const uint8_t* raw_i = d_raw + (size_t)lo * 2 * n;
        RET_IF(ensure(c, L.dec, (size_t)S * nd * sizeof(cplx)));
        // staggered lanes: this lane's front kernel starts when the previous lane's has finished -- the bandwidth-bound front kernels
        // then follow one another instead of competing, and each runs beside the compute-bound stages of the lanes ahead of it.
        // Measured (round 4, NOTES_r04.md): 128 / 256 / 512 / 1 024 / 2 048 streams 0.345 / 0.562 / 1.002 / 1.807 / 3.629 ms staggered
        // against 0.349 / 0.554 / 1.002 / 1.874 / 3.715 together: worth it from 256 streams per lane on.
        const bool stagger = nl > 1 && d / nl >= 256;   // (one decision for all lanes of the call)
        if (stagger) {
            if (!L.front_done) HIPCHK(c, hipEventCreateWithFlags(&L.front_done, hipEventDisableTiming));
            if (i > 0) HIPCHK(c, hipStreamWaitEvent(L.stream, c->lanes[i - 1].front_done, 0));
        }
        RET_IF(front_fused(c, raw_i, S, n, (const double*)c->coef.p, ntaps, decim, (cplx*)L.dec.p, nd));  // :107,110,117
        if (stagger) HIPCHK(c, hipEventRecord(L.front_done, L.stream));
        RET_IF(coarse(c, S, (const cplx*)L.dec.p, nd, nd, dec_ratio, ov, true, n, decim));         // :117 (+ state init, fine setup)
        Source src{SRC_RAW, raw_i, 2 * n, nullptr, 0, (const double*)c->coef.p, ntaps};
        c->cf_lane = cf_all + lo;
        ChainOut co{d_table + (size_t)lo * GSMCAL_TABLE_COLS, d_pos_info ? d_pos_info + (size_t)lo * 2 * MAXROWS : nullptr,
                    d_r_len ? d_r_len + lo : nullptr, false};
        RET_IF(run_fine(c, S, src, 0, g, H, true, 2, len_ts, &co));                         // :118 (+ SCH window setup; fused: :118-124)
        if (!co.fused) {
            RET_IF(run_sch(c, S, src, 2, g, H, len_ts, true, 3));                           // :119 (+ post-SCH window setup)
            RET_IF(run_post(c, S, src, 3, g, H, true, co.table, co.pos_info_out, co.r_len_out));   // :120, :123-124
        }
        if (d_r_correct) RET_IF(launch_r_correct(c, L, src, raw_i, S, n, ntaps, d_r_correct + (size_t)2 * lo * n));
    }
    c->cf_lane = nullptr;
    RET_IF(join_lanes(c, nl));
    return 0;
    };
    const unsigned long long fused_before = c->n_fused_launches;
    RET_IF(run_maybe_graph(c, pick_slot(c, c->g_calib, key), key, enqueue, plan_lanes(c, d) > 1));
    c->no_fuse_now = false;
    if (c->n_fused_launches != fused_before) record_fused_call(c, d_raw, d, n, ntaps, len_ts, d_table, d_pos_info, d_r_correct, d_r_len);
    plan_lanes(c, d);          // lane bookkeeping for gsmcal_last_batch_details (a replay does not run `enqueue`)
    c->cur = &c->lanes[0];
    c->last_S = d;
    return 0;
}

int gsmcal_calibrate_batch(gsmcal_ctx* c, const uint8_t* raw, int d, long n, const double* coef, int ntaps,
                           const double* sch_ts, int len_ts, const double* carrier_freq, double* table,
                           double* pos_info, double* r_correct, long* r_len) {
    if (!c || !raw || !table || d < 1 || n < 1) return GSMCAL_E_ARG;
    ENTER(c);
    const Stage io[] = {STAGE(misc, (size_t)2 * n * d, raw, nullptr, 0),
                        STAGE(table, (size_t)d * GSMCAL_TABLE_COLS * sizeof(double), nullptr, table, 0),
                        STAGE(posinfo, (size_t)d * 2 * MAXROWS * sizeof(double), nullptr, pos_info, 0),
                        STAGE(rlen, (size_t)d * sizeof(long), nullptr, r_len, 0),
                        STAGE(arr_out, r_correct ? (size_t)d * n * sizeof(cplx) : 0, nullptr, r_correct, 0)};
    RET_IF(stage_up(c, io));
    RET_IF(gsmcal_calibrate_batch_dev(c, (const uint8_t*)c->misc.p, d, n, coef, ntaps, sch_ts, len_ts, carrier_freq,
                                      (double*)c->table.p, (double*)c->posinfo.p,
                                      r_correct ? (double*)c->arr_out.p : nullptr, (long*)c->rlen.p));
    RET_IF(pipe_join(c));                      // (a pipelined context: the copies below wait for this call like for any other)
    if (!c->fused_calls.empty()) {             // (the fused tail ran: had it timed out, the call runs again as four launches before anything is copied)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        RET_IF(fused_recover(c));
    }
    return stage_down(c, io);
}

