// ufm_map_host.h -- the host side of keeping the raster: the one way a patch takes (Engine::route_patch, acting on plan_patch of
// ufm_patch_route.h), held and deferred patches, the footprint, the census, the sensor reveal, surveys, layers, a new raster from bytes
// or from a bitmap, and the reads of all of these.  DESIGN.md section 5.1.
// (a piece of ufm_engine.hip, the engine's one translation unit: included there behind ufm_host.h, inside its anonymous namespace)
#pragma once

constexpr PatchRouteConfig PATCH_ROUTE_CONFIG{PATCH_MULTI, 4096, REGION_HELD_EDGE, Engine::LAZY_SLOTS};   // (hold_edge: what the block kernel's divisions and change mask are made for, ufm_region_rect.h)

// ---- what is held or deferred, applied -----------------------------------------------------------------------------------------
int Engine::flush_deferred() {       // a single planner's host patches, then a batch's deferred device patches
    { int rc = flush_lazy(); if (rc != UFM_OK) return rc; }
    return flush_deferred_only();
}
int Engine::flush_deferred_only() {
    if (deferred.empty()) return UFM_OK;
    PatchMulti a{};
    a.n = (int)deferred.size();
    for (int i = 0; i < a.n; ++i) {
        const DeferredPatch &d = deferred[i];
        put_rect(a.rect[i], PatchRect{d.m, d.x, d.y, d.w, d.h});
        a.ptr[i] = d.ptr;
    }
    deferred.clear();
    with_elements(algo, [&](auto nodes) { k_patch_multi<nodes()><<<a.n, 1024, 0, stream>>>(P, a, d_pmask.dev); });
    HIPCHK(hipGetLastError());
    return UFM_OK;
}
int Engine::ensure_pmask(size_t need) {
    if (need <= d_pmask.cap) return UFM_OK;
    { int rc = flush_deferred_only(); if (rc != UFM_OK) return rc; }      // (their launch writes the old buffer)
    return d_pmask.reserve(stream, need);
}
// the held host patches, applied the ordinary way (one k_patch_small each, reading the pinned slot), in the order they came
int Engine::flush_lazy() {
    if (lazy.empty()) return UFM_OK;
    { int rc = ensure_pmask(patch_mask_bytes(PATCH_ROUTE_CONFIG, 0)); if (rc != UFM_OK) return rc; }
    for (const LazyPatch &p : lazy) {
        patch_small(p.m, h_lazy + (size_t)p.slot * 4096, p.x, p.y, p.w, p.h);
        lazy_dirty[p.slot] = true;         // (read by a kernel that is only queued: hold_host_patch waits for the stream before it writes the slot again)
    }
    lazy.clear();
    HIPCHK(hipGetLastError());
    return UFM_OK;
}
// way Hold: the bytes into the next pinned slot, the rectangle to the pending ones
int Engine::hold_host_patch(const PatchRect &r, const uint8_t *host_patch) {
    { int rc = h_lazy.ensure((size_t)LAZY_SLOTS * 4096, Pin::Mapped); if (rc != UFM_OK) return rc; }
    // (a slot is free again when the step that consumed its patch has returned -- step() is synchronous -- or when flush_lazy() has run and the
    //  stream has been waited for; slots are handed out in order, so the one after the last held patch's is the oldest)
    const int slot = lazy.empty() ? (lazy_next % LAZY_SLOTS) : ((lazy.back().slot + 1) % LAZY_SLOTS);
    if (lazy_dirty[slot]) { HIPCHK(hipStreamSynchronize(stream)); for (bool &d : lazy_dirty) d = false; }
    std::memcpy(h_lazy + (size_t)slot * 4096, host_patch, (size_t)r.w * r.h);
    __atomic_thread_fence(__ATOMIC_RELEASE);
    lazy.push_back({r.m, r.x, r.y, r.w, r.h, slot});
    lazy_next = slot + 1;
    pending.push_back(r);
    return UFM_OK;
}

// ---- the way of a patch ----------------------------------------------------------------------------------------------------------
PatchSwitches Engine::patch_switches(int m) const {
    return PatchSwitches{cs.on, cs.mh, cs.mw, cs.ar, cs.ac, census_on, n_layers, nmaps, defer_patches, lazy_patches, use_region, fuse_control,
                         spin_wait, L, W, allocated && m >= 0 && m < nmaps && maps[m].have_map};
}
PatchPlan Engine::patch_plan(PatchSource source, bool host_bytes, int k, const PatchRect &r) const {
    bool same_map = false;
    for (const DeferredPatch &d : deferred) same_map = same_map || d.m == r.m;
    return plan_patch(PATCH_ROUTE_CONFIG, patch_switches(r.m), PatchQueue{(int)pending.size(), (int)lazy.size(), (int)deferred.size(), same_map},
                      PatchRequest{source, host_bytes, k, sensor.mh, sensor.mw, r});
}
// the caller's host bytes into the staging buffer: device bytes when the stream gets there
int Engine::stage_host_patch(const uint8_t *src, size_t n) {
    if (n > d_patch.cap) { int rc = d_patch.reserve(stream, n, true); if (rc != UFM_OK) return rc; }
    else HIPCHK(hipStreamSynchronize(stream));   // staging buffers are reused
    std::memcpy(d_patch.pinned, src, n);
    HIPCHK(hipMemcpyAsync(d_patch.dev, d_patch.pinned, n, hipMemcpyHostToDevice, stream));
    return UFM_OK;
}
// what the plan asks for in front of the patch: what goes to the raster first, the scratch
int Engine::patch_room(const PatchPlan &p) {
    if (p.flush_held) { int rc = flush_lazy(); if (rc != UFM_OK) return rc; }
    { int rc = d_lcomp.reserve(stream, p.lcomp_bytes); if (rc != UFM_OK) return rc; }
    { int rc = d_cs_patch.reserve(stream, p.cs_bytes); if (rc != UFM_OK) return rc; }
    { int rc = ensure_pmask(p.pmask_bytes); if (rc != UFM_OK) return rc; }
    if (p.flush_deferred) { int rc = flush_deferred_only(); if (rc != UFM_OK) return rc; }
    return UFM_OK;
}
// Every patch, stream-ordered.  Everything that can fail -- the staging copy, applying what is held, the growth of the buffers -- comes
// before the first write to any store: a call that returns an error has left the layers and both rasters as they were.
int Engine::route_patch(PatchSource source, bool host_bytes, int k, const uint8_t *bytes, const PatchRect &r) {
    const PatchPlan p = patch_plan(source, host_bytes, k, r);
    if (p.way == PatchWay::Invalid) return UFM_ERR_INVALID;
    if (p.way == PatchWay::Hold) return hold_host_patch(r, bytes);
    if (p.stage) {
        { int rc = stage_host_patch(bytes, (size_t)r.w * r.h); if (rc != UFM_OK) return rc; }
        bytes = d_patch.dev;
    }
    { int rc = patch_room(p); if (rc != UFM_OK) return rc; }
    if (p.compose) {      // into layer k, the maximum over the layers into the dense composed patch
        { int rc = compose_layer(k, bytes, r); if (rc != UFM_OK) return rc; }
        bytes = d_lcomp.dev;
    }
    const PatchRect &a = p.applied;
    if (p.raw) {          // into the raw store, the grown rectangle dilated into the scratch patch
        k_raw_store<<<(r.w * r.h + 255) / 256, 256, 0, stream>>>(d_raw + (size_t)r.m * P.cstride, W, bytes, r.x, r.y, r.w, r.h);
        cspace_dilate(r.m, d_cs_patch.dev, a.w, a);
        HIPCHK(hipGetLastError());
        bytes = d_cs_patch.dev;
    }
    if (p.way == PatchWay::Defer) {
        // (a batch only: the patch kernel of a single map runs while the host prepares the step -- applying it inside the
        //  replan's block kernel instead was tried and saved nothing, it only made that kernel longer)
        deferred.push_back({a.m, a.x, a.y, a.w, a.h, bytes});
        pending.push_back(a);
        return UFM_OK;
    }
    // the patch kernels detect the cells of the planning raster that really changed, seed from them and keep the cost windows in step
    const int n = a.w * a.h;
    if (p.census) { census_patch(a.m, bytes, a.x, a.y, a.w, a.h); census_publish(); }   // (reads the old bytes)
    if (p.small) {
        patch_small(a.m, bytes, a.x, a.y, a.w, a.h);
    } else {
        k_patch_apply<<<(n + 255) / 256, 256, 0, stream>>>(P, a.m, bytes, d_pmask.dev, a.x, a.y, a.w, a.h);
        const int ne = (a.w + 1) * (a.h + 1);
        with_elements(algo, [&](auto nodes) { k_patch_seed<nodes()><<<(ne + 255) / 256, 256, 0, stream>>>(P, a.m, d_pmask.dev, a.x, a.y, a.w, a.h); });
    }
    HIPCHK(hipGetLastError());
    pending.push_back(a);
    return UFM_OK;
}
int engine_patch(Engine *e, int m, const uint8_t *src, bool on_device, int x, int y, int w, int h) {
    if (!e || !src) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    return e->route_patch(on_device ? PatchSource::Device : PatchSource::Host, !on_device, 0, src, PatchRect{m, x, y, w, h});
}

// ---- C-space inflation: planning raster == dilate(raw raster), kept at a cost proportional to the patch ----
// (the one place that knows which kind of footprint is set: everything else works on the support, cs)
void Engine::cspace_dilate(int m, uint8_t *out, int pitch, const PatchRect &r) {
    if (csl.n > 1) {
        CspaceGradedJob j{};
        j.raw = d_raw + (size_t)m * P.cstride; j.out = out;
        j.L = L; j.W = W; j.x0 = r.x; j.y0 = r.y; j.h = r.h; j.w = r.w; j.pitch = pitch;
        j.mh = cs.mh; j.mw = cs.mw; j.ar = cs.ar; j.ac = cs.ac; j.nl = csl.n;
        for (int l = 0; l < csl.n; ++l) {
            j.drop[l] = csl.drop[l];
            for (int a = 0; a < CSPACE_MAX; ++a) j.rows[l][a] = csl.rows[l][a];
        }
        k_cspace_dilate_graded<<<dim3((r.w + CS_TC - 1) / CS_TC, (r.h + CS_TR - 1) / CS_TR), 256, 0, stream>>>(j);
        return;
    }
    CspaceJob j{};
    j.raw = d_raw + (size_t)m * P.cstride; j.out = out;
    j.L = L; j.W = W; j.x0 = r.x; j.y0 = r.y; j.h = r.h; j.w = r.w; j.pitch = pitch;
    j.mh = cs.mh; j.mw = cs.mw; j.ar = cs.ar; j.ac = cs.ac;
    for (int a = 0; a < CSPACE_MAX; ++a) j.rows[a] = cs.rows[a];
    k_cspace_dilate<<<dim3((r.w + CS_TC - 1) / CS_TC, (r.h + CS_TR - 1) / CS_TR), 256, 0, stream>>>(j);
}
// ufm_set_cspace / ufm_batch_set_cspace: a property of the vehicle, set before the first raster
int engine_set_cspace(Engine *e, const uint8_t *mask, int mw, int mh, int ar, int ac) {
    if (!e) return UFM_ERR_INVALID;
    for (const MapState &ms : e->maps) if (ms.have_map) return UFM_ERR_INVALID;
    if (!cspace_pack(mask, mw, mh, ar, ac, &e->cs)) return UFM_ERR_INVALID;
    e->csl = CspaceLevels{};     // (the last footprint call before the first raster wins: a graded one is replaced)
    // (arrays without a map -- a ufm_set_map that failed after its allocation -- were sized without the raw store: the next one allocates anew)
    if (e->allocated) { HIPCHK(hipSetDevice(e->device)); e->release(); }
    return UFM_OK;
}
// ufm_set_cspace_graded / ufm_batch_set_cspace_graded: the same property, with a drop per cell.  The support goes where the flat mask
// goes; drops that are all 0 leave one level and the state ufm_set_cspace would leave for the mask drop != 255 -- the flat kernel runs.
int engine_set_cspace_graded(Engine *e, const uint8_t *drop, int mw, int mh, int ar, int ac) {
    if (!e) return UFM_ERR_INVALID;
    for (const MapState &ms : e->maps) if (ms.have_map) return UFM_ERR_INVALID;
    CspaceMask support;
    CspaceLevels levels;
    if (!cspace_graded_pack(drop, mw, mh, ar, ac, &support, &levels)) return UFM_ERR_INVALID;
    e->cs = support;
    e->csl = levels.n > 1 ? levels : CspaceLevels{};
    if (e->allocated) { HIPCHK(hipSetDevice(e->device)); e->release(); }
    return UFM_OK;
}

// ---- the cost census: hist[v] == number of cells of P.cost with value v, per map ----
void Engine::census_build(int m) {
    uint32_t *hist = d_census + (size_t)m * CENSUS_BINS;
    (void)hipMemsetAsync(hist, 0, sizeof(uint32_t) * CENSUS_BINS, stream);
    const CensusBuildJob j{P.cost + (size_t)m * P.cstride, P.cstride, hist};
    k_census_build<<<census_build_grid(census_split(reinterpret_cast<uintptr_t>(j.cost), j.n).nvec), CENSUS_THREADS, 0, stream>>>(j);
}
void Engine::census_patch(int m, const uint8_t *dev_patch, int x, int y, int w, int h) {
    const CensusPatchJob j{P.cost + (size_t)m * P.cstride, dev_patch, d_census + (size_t)m * CENSUS_BINS, W, x, y, w, h};
    k_census_patch<<<census_patch_grid(w * h), CENSUS_THREADS, 0, stream>>>(j);
}
// the published range as of the last build or patch queued: the host waits for that copy's sequence number (nothing is held while the census is on)
int Engine::census_minmax(int *mn, int *mx) {
    if (!census_on) return UFM_ERR_INVALID;
    { int rc = wait_flag(h_cen.flag(), cen_seq); if (rc != UFM_OK) return rc; }
    *mn = h_cen->v[0]; *mx = h_cen->v[1];
    return UFM_OK;
}
// ufm_track_costs / ufm_batch_track_costs.  On, with maps already set: what is held is applied and the counters are built from the rasters
// as they stand.  Off frees everything; refused while "auto_multiplier" is 1 (the step would have nothing to take).
int engine_track_costs(Engine *e, int enable) {
    if (!e) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    if (!enable) {
        if (!e->census_on) return UFM_OK;
        if (e->auto_multiplier) return UFM_ERR_INVALID;
        HIPCHK(hipStreamSynchronize(e->stream));
        e->census_free();
        return UFM_OK;
    }
    if (e->census_on) return UFM_OK;
    if (e->allocated) { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }
    const int rc = [&]() -> int {
        { int ra = e->d_census.alloc((size_t)CENSUS_BINS * e->nmaps); if (ra != UFM_OK) return ra; }
        { int ra = e->h_cen.alloc(); if (ra != UFM_OK) return ra; }
        e->cen_seq = 0;
        HIPCHK(hipMemsetAsync(e->d_census, 0, sizeof(uint32_t) * CENSUS_BINS * e->nmaps, e->stream));
        for (int m = 0; m < e->nmaps; ++m) if (e->allocated && e->maps[m].have_map) e->census_build(m);
        e->census_publish();
        HIPCHK(hipGetLastError());
        return UFM_OK;
    }();
    if (rc != UFM_OK) { (void)hipStreamSynchronize(e->stream); e->census_free(); return rc; }
    e->census_on = true;
    return UFM_OK;
}
// the counters of map m, as they are once everything queued has run
int engine_read_census(Engine *e, int m, uint32_t out[CENSUS_BINS]) {
    if (!e || !e->census_on || !e->allocated || m < 0 || m >= e->nmaps || !e->maps[m].have_map) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }
    HIPCHK(hipMemcpyAsync(out, e->d_census + (size_t)m * CENSUS_BINS, sizeof(uint32_t) * CENSUS_BINS, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return UFM_OK;
}

// ---- cost layers: the caller's raster == max over the layers, kept at a cost proportional to the patch ----
// profiling: the events the next layer kernel's dispatch carries (null while profiling is off)
int Engine::layer_events(hipEvent_t *e0, hipEvent_t *e1) {
    *e0 = *e1 = nullptr;
    lay_timed = false;
    if (!profiling) return UFM_OK;
    { int rc = lay_ev.ensure(); if (rc != UFM_OK) return rc; }
    *e0 = lay_ev[0]; *e1 = lay_ev[1];
    lay_timed = true;
    return UFM_OK;
}
// the bytes into layer k, the maximum over the layers of that rectangle into d_lcomp.  The whole map (ufm_set_layer): a copy and the vector kernel.
int Engine::compose_layer(int k, const uint8_t *dev_patch, const PatchRect &r) {
    hipEvent_t e0, e1;
    { int rc = layer_events(&e0, &e1); if (rc != UFM_OK) return rc; }
    const size_t n = (size_t)r.w * r.h;
    if (layers_rect_is_map(r.x, r.y, r.w, r.h, L, W)) {
        HIPCHK(hipMemcpyAsync(layer_ptr(k, r.m), dev_patch, n, hipMemcpyDeviceToDevice, stream));
        LayerComposeAllJob j{};
        for (int l = 0; l < n_layers; ++l) j.layer[l] = layer_ptr(l, r.m);
        j.out = d_lcomp.dev; j.cells = n; j.n = n_layers;
        const LayersSplit s = layers_split(reinterpret_cast<uintptr_t>(j.out), n);
        launch(k_layer_compose_all, dim3(layers_all_grid(s.nvec)), dim3(LAYERS_THREADS), stream, e0, e1, j);
    } else {
        LayerComposeJob j{};
        for (int l = 0; l < n_layers; ++l) j.layer[l] = layer_ptr(l, r.m);
        j.patch = dev_patch; j.out = d_lcomp.dev;
        j.n = n_layers; j.k = k; j.W = W; j.x = r.x; j.y = r.y; j.w = r.w; j.h = r.h;
        launch(k_layer_compose, dim3(layers_rect_grid(r.w * r.h)), dim3(LAYERS_THREADS), stream, e0, e1, j);
    }
    HIPCHK(hipGetLastError());
    return UFM_OK;
}
// ufm_patch_layer* / ufm_batch_patch_layer*
int engine_patch_layer(Engine *e, int m, int k, const uint8_t *src, bool on_device, int x, int y, int w, int h) {
    if (!e || !src) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    return e->route_patch(PatchSource::Layer, !on_device, k, src, PatchRect{m, x, y, w, h});
}
// ufm_set_layer*: layer k wholesale, a whole-map patch -- not a set_map: the field is kept and the next step replans
int engine_set_layer(Engine *e, int m, int k, const uint8_t *src, bool on_device, int width, int length) {
    if (!e || !e->allocated || width != e->W || length != e->L) return UFM_ERR_INVALID;
    return engine_patch_layer(e, m, k, src, on_device, 0, 0, width, length);
}
// ufm_set_layers / ufm_batch_set_layers: a property of the handle, set before the first raster
int engine_set_layers(Engine *e, int n) {
    if (!e || !layers_count_ok(n)) return UFM_ERR_INVALID;
    for (const MapState &ms : e->maps) if (ms.have_map) return UFM_ERR_INVALID;
    // (arrays without a map -- a ufm_set_map that failed after its allocation -- were sized for the old count: the next one allocates anew)
    if (e->allocated) { HIPCHK(hipSetDevice(e->device)); e->release(); }
    e->n_layers = n;
    return UFM_OK;
}
int engine_read_layer(Engine *e, int m, int k, uint8_t *out) {
    if (!e || !out || m < 0 || m >= e->nmaps || !e->allocated || !e->maps[m].have_map || !layers_index_ok(k, e->n_layers)) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(out, e->layer_ptr(k, m), e->P.cstride, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return UFM_OK;
}

// ---- surveys: what the sensor would see of layer k of map m, for the raster that map has (one layer: k = 0, the map) ----
int Engine::survey_alloc(int k) {
    if (d_lsurvey[k]) return UFM_OK;
    { int rc = d_lsurvey[k].alloc(P.cstride * nmaps); if (rc != UFM_OK) return rc; }
    have_lsurvey[k].assign((size_t)nmaps, 0);
    return UFM_OK;
}
// ufm_set_layer_survey* / ufm_batch_set_layer_survey*; k = 0 is ufm_set_survey*, with or without layers
int engine_set_layer_survey(Engine *e, int m, int k, const uint8_t *src, bool on_device, int width, int length) {
    if (!e || !src || m < 0 || m >= e->nmaps || !e->allocated || !e->maps[m].have_map || width != e->W || length != e->L) return UFM_ERR_INVALID;
    if (k != 0 && !layers_index_ok(k, e->n_layers)) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->survey_alloc(k); if (rc != UFM_OK) return rc; }
    HIPCHK(hipMemcpyAsync(e->d_lsurvey[k] + (size_t)m * e->P.cstride, src, e->P.cstride, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));      // (the caller's buffer is free again when the call returns)
    e->reveal_busy = false;
    e->have_lsurvey[k][m] = 1;
    return UFM_OK;
}
// ufm_read_layer_survey (layer_call: only with layers, k one of them) and ufm_read_survey (k = 0, with or without)
int engine_read_layer_survey(Engine *e, int m, int k, uint8_t *host_survey, bool layer_call = true) {
    if (!e || !host_survey || m < 0 || m >= e->nmaps || !e->allocated) return UFM_ERR_INVALID;
    if ((layer_call ? !layers_index_ok(k, e->n_layers) : k != 0) || !((e->layer_surveys(m) >> k) & 1)) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(host_survey, e->d_lsurvey[k] + (size_t)m * e->P.cstride, e->P.cstride, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return UFM_OK;
}

// ---- the sensor reveal: a move uncovers the surveys' field of view, as a patch made on the device ----
// ufm_set_sensor / ufm_batch_set_sensor: the field of view, set or replaced between any two calls; needs no map
int engine_set_sensor(Engine *e, const uint8_t *mask, int mw, int mh, int ar, int ac) {
    if (!e) return UFM_ERR_INVALID;
    SensorShape s;
    if (!sensor_pack(mask, mw, mh, ar, ac, &s)) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    {   // (each allocated once: a call that fails half way leaves owned buffers, and the next one makes the rest)
        int rc = e->d_sensor.ensure((size_t)SENSOR_MAX * SENSOR_MAX);
        if (rc == UFM_OK) rc = e->d_reveal_cnt.ensure((size_t)e->nmaps);
        if (rc == UFM_OK) rc = e->h_centres.ensure(3 * (size_t)e->nmaps, Pin::Mapped);
        if (rc != UFM_OK) return rc;
    }
    // (a reveal that is only queued reads the old mask: wait for it, then replace the bytes)
    HIPCHK(hipStreamSynchronize(e->stream));
    e->reveal_busy = false;
    HIPCHK(hipMemcpy(e->d_sensor, mask, (size_t)mw * mh, hipMemcpyHostToDevice));
    e->sensor = s;
    return UFM_OK;
}
// everything a reveal of these centres ([nmaps][2], row < 0: skipped) needs; nothing is launched or written.  Every map that is not
// skipped needs a survey: of the map with one layer, of any layer with more.
int Engine::reveal_check(const int32_t *centres) const {
    if (!centres || !sensor.set || !allocated || (n_layers == 1 && !d_lsurvey[0])) return UFM_ERR_INVALID;
    for (int m = 0; m < nmaps; ++m) {
        if (centres[2 * m] < 0) continue;
        if (!maps[m].have_map || !layer_surveys(m) || !sensor_centre_ok(centres[2 * m], centres[2 * m + 1], L, W)) return UFM_ERR_INVALID;
    }
    return UFM_OK;
}
// One kernel for all maps -- k_reveal, with layers k_reveal_layers, which uncovers every layer that has a survey --, then every map's
// slot through route_patch().  As there, whatever can fail comes before the first write to a raster.
int Engine::reveal(const int32_t *centres) {
    { int rc = reveal_check(centres); if (rc != UFM_OK) return rc; }
    auto slot_rect = [&](int m) {
        const SensorRect r = sensor_place(centres[2 * m], centres[2 * m + 1], sensor.mh, sensor.mw, sensor.ar, sensor.ac, L, W);
        return PatchRect{m, r.x, r.y, r.w, r.h};
    };
    int first = -1;
    for (int m = nmaps - 1; m >= 0; --m) if (centres[2 * m] >= 0) first = m;
    if (first < 0) return UFM_OK;
    // held patches first, in order -- and a deferred one may point into the slots the kernel is about to overwrite
    { int rc = flush_deferred(); if (rc != UFM_OK) return rc; }
    const size_t stride = sensor_slot_stride(sensor.mw, sensor.mh);
    { int rc = d_reveal.reserve(stream, stride * (size_t)nmaps); if (rc != UFM_OK) return rc; }
    { int rc = patch_room(patch_plan(PatchSource::RevealSlot, false, 0, slot_rect(first))); if (rc != UFM_OK) return rc; }   // (one size for every slot)
    const bool layers = n_layers > 1;
    if (reveal_busy) { HIPCHK(hipStreamSynchronize(stream)); reveal_busy = false; }
    for (int m = 0; m < nmaps; ++m) {
        int32_t *c = h_centres + (layers ? 3 : 2) * m;
        c[0] = centres[2 * m]; c[1] = centres[2 * m + 1];
        if (layers) c[2] = layer_surveys(m);
    }
    __atomic_thread_fence(__ATOMIC_RELEASE);
    HIPCHK(hipMemsetAsync(d_reveal_cnt, 0, sizeof(unsigned int) * nmaps, stream));
    const dim3 grid(sensor_grid_x(sensor.mw, sensor.mh), nmaps), block(SENSOR_THREADS);
    if (layers) {
        RevealLayersJob j{};
        j.mask = d_sensor; j.layers = d_layers; j.cur = cs.on ? d_raw : P.cost; j.slots = d_reveal.dev; j.count = d_reveal_cnt; j.centres = h_centres;
        for (int k = 0; k < n_layers; ++k) j.survey[k] = d_lsurvey[k];
        j.cstride = P.cstride; j.lstride = lstride; j.slot_stride = stride;
        j.n = n_layers; j.nmaps = nmaps; j.L = L; j.W = W; j.mh = sensor.mh; j.mw = sensor.mw; j.ar = sensor.ar; j.ac = sensor.ac;
        hipEvent_t e0, e1;
        { int rc = layer_events(&e0, &e1); if (rc != UFM_OK) return rc; }
        launch(k_reveal_layers, grid, block, stream, e0, e1, j);
    } else {
        RevealJob j{};
        j.mask = d_sensor; j.survey = d_lsurvey[0]; j.cur = cs.on ? d_raw : P.cost; j.slots = d_reveal.dev; j.count = d_reveal_cnt; j.centres = h_centres;
        j.cstride = P.cstride; j.slot_stride = stride;
        j.L = L; j.W = W; j.mh = sensor.mh; j.mw = sensor.mw; j.ar = sensor.ar; j.ac = sensor.ac;
        launch(k_reveal, grid, block, stream, nullptr, nullptr, j);
    }
    HIPCHK(hipGetLastError());
    reveal_busy = true;
    for (int m = first; m < nmaps; ++m) {
        if (centres[2 * m] < 0) continue;
        const int rc = route_patch(PatchSource::RevealSlot, false, 0, d_reveal.dev + stride * (size_t)m, slot_rect(m));
        if (rc != UFM_OK) return rc;
    }
    return UFM_OK;
}
// the counts of the last reveal, once the stream has run: changed[m], 0 for a map that was skipped
int Engine::reveal_counts(const int32_t *centres, uint64_t *changed) {
    std::vector<unsigned int> cnt((size_t)nmaps, 0u);
    bool any = false;
    for (int m = 0; m < nmaps; ++m) any = any || centres[2 * m] >= 0;
    if (any) HIPCHK(hipMemcpyAsync(cnt.data(), d_reveal_cnt, sizeof(unsigned int) * nmaps, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    reveal_busy = false;
    for (int m = 0; m < nmaps; ++m) changed[m] = centres[2 * m] >= 0 ? cnt[m] : 0u;
    return UFM_OK;
}

// ---- a new raster ------------------------------------------------------------------------------------------------------------------
// What ufm_set_map* and ufm_set_image* share: map m gets a new raster of width x length.  fill(dst) queues whatever writes the caller's
// raster to dst -- map m's slot of the raw store with a footprint, of the planning raster without -- and does everything of its own that
// can fail before its first write; the rest is the same for both: held patches first, (re)allocation under the batch's one-size rule,
// the dilation, the census, the cost windows, the mean traversable cost, an empty step-delta baseline, the goal's validity.
template <class Fill> int engine_new_raster(Engine *e, int m, int width, int length, Fill &&fill) {
    HIPCHK(hipSetDevice(e->device));
    if (e->allocated) { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }   // (patches held back belong before the new raster)
    if (!e->allocated || width != e->W || length != e->L) {
        bool others = false;
        for (int k = 0; k < e->nmaps; ++k) if (k != m && e->maps[k].have_map) others = true;
        if (e->allocated && others) return UFM_ERR_INVALID;   // all maps of a batch share one size
        int rc = e->alloc(width, length);
        if (rc != UFM_OK) return rc;
        if (e->census_on) HIPCHK(hipMemsetAsync(e->d_census, 0, sizeof(uint32_t) * CENSUS_BINS * e->nmaps, e->stream));   // (no map has a raster)
    }
    // (a footprint: the input is the raw raster -- kept, and dilated into the planning raster before anything reads that one)
    { int rc = fill((e->cs.on ? e->d_raw : e->P.cost) + (size_t)m * e->P.cstride); if (rc != UFM_OK) return rc; }
    if (e->n_layers > 1) {   // (layers: the argument is layer 0, the others start at zero -- rock_aboundance_l = np.zeros(...), run_test.py:102)
        HIPCHK(hipMemcpyAsync(e->layer_ptr(0, m), (e->cs.on ? e->d_raw : e->P.cost) + (size_t)m * e->P.cstride, e->P.cstride, hipMemcpyDeviceToDevice, e->stream));
        for (int k = 1; k < e->n_layers; ++k) HIPCHK(hipMemsetAsync(e->layer_ptr(k, m), 0, e->P.cstride, e->stream));
    }
    if (e->cs.on) e->cspace_dilate(m, e->P.cost + (size_t)m * e->P.cstride, width, PatchRect{m, 0, 0, width, length});
    if (e->census_on) { e->census_build(m); e->census_publish(); }      // (the planning raster is final; published by the wait below)
    k_cost_windows<<<2048, 256, 0, e->stream>>>(e->P, m);
    {   // mean traversable cost -> default ordering band
        unsigned long long *d_acc = reinterpret_cast<unsigned long long *>(e->d_scratch);
        HIPCHK(hipMemsetAsync(d_acc, 0, 2 * sizeof(unsigned long long), e->stream));
        k_cost_stats<<<512, 256, 0, e->stream>>>(e->P.cost + (size_t)m * e->P.cstride, (size_t)width * length, e->thr_uchar, d_acc);
        unsigned long long *h_acc = e->scratch.acc;
        HIPCHK(hipMemcpyAsync(h_acc, d_acc, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (h_acc[1] > 0) e->mean_cost = (float)((double)h_acc[0] / (double)h_acc[1]);
    }
    if (e->track) { int rc = e->track_reset(m); if (rc != UFM_OK) return rc; }   // a new raster: the caller's view of this map starts empty again
    e->maps[m].have_map = true;   // initialize_graph = false, ReplannerBase.h:87
    // goal element validity depends on the map size
    MapState &ms = e->maps[m];
    if (ms.goal_set) ms.goal_elem_valid = ms.goal_ex >= 0 && ms.goal_ey >= 0 && ms.goal_ex < e->P.EX && ms.goal_ey < e->P.EY;
    return UFM_OK;
}

int engine_set_map(Engine *e, int m, const uint8_t *src, bool on_device, int width, int length) {
    if (!e || !src || m < 0 || m >= e->nmaps || width <= 0 || length <= 0) return UFM_ERR_INVALID;
    return engine_new_raster(e, m, width, length, [&](uint8_t *dst) -> int {
        HIPCHK(hipMemcpyAsync(dst, src, (size_t)width * length, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
        return UFM_OK;
    });
}

// ufm_set_image* / ufm_batch_set_image*: the bitmap becomes map m's raster AND its survey (k_prepare, one launch).  The survey's array and
// the staging buffer are seen to before k_prepare writes either raster; the wait at the end of engine_new_raster() is what frees the
// caller's buffer -- and the staging buffer for the next map.
int engine_set_image(Engine *e, int m, const uint8_t *src, bool on_device, int width, int length, const uint16_t *taps, int ntaps, int penalty) {
    PrepTaps k;
    if (!e || !src || m < 0 || m >= e->nmaps || !prep_args_valid(taps, ntaps, width, length, penalty) || !prep_pack(taps, ntaps, &k)) return UFM_ERR_INVALID;
    if (e->allocated && (width != e->W || length != e->L))       // (the one-size rule of a batch, before anything is flushed or freed)
        for (int j = 0; j < e->nmaps; ++j) if (j != m && e->maps[j].have_map) return UFM_ERR_INVALID;
    bool timed = false;
    const int rc = engine_new_raster(e, m, width, length, [&](uint8_t *dst) -> int {
        const size_t n = (size_t)width * length, all = e->P.cstride * e->nmaps;
        { int rc2 = e->survey_alloc(0); if (rc2 != UFM_OK) return rc2; }
        uint8_t *survey = e->d_lsurvey[0];
        const uint8_t *image = src;
        if (!on_device || prep_overlap(src, n, e->P.cost, all) || prep_overlap(src, n, survey, all) || (e->cs.on && prep_overlap(src, n, e->d_raw, all))) {
            { int rc2 = e->d_image.reserve(e->stream, n); if (rc2 != UFM_OK) return rc2; }
            HIPCHK(hipMemcpyAsync(e->d_image.dev, src, n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
            image = e->d_image.dev;
        }
        PrepareJob j{};
        j.src = image; j.out_l = dst; j.out_h = survey + (size_t)m * e->P.cstride;
        j.W = width; j.L = length; j.penalty = penalty;
        j.wide_in = width % 4 == 0 && prep_aligned4(j.src);
        j.wide_out = width % 4 == 0 && prep_aligned4(j.out_l) && prep_aligned4(j.out_h);
        j.taps = k;
        timed = e->profiling;
        if (timed) { int rc2 = e->prep_ev.ensure(); if (rc2 != UFM_OK) return rc2; }
        launch(k_prepare, dim3(prep_grid_x(width), prep_grid_y(length)), dim3(PREP_THREADS), e->stream, timed ? e->prep_ev[0] : nullptr,
               timed ? e->prep_ev[1] : nullptr, j);
        HIPCHK(hipGetLastError());
        e->have_lsurvey[0][m] = 1;
        return UFM_OK;
    });
    if (rc != UFM_OK) return rc;
    e->reveal_busy = false;                  // (the call has waited for the stream)
    if (timed) HIPCHK(hipEventElapsedTime(&e->prep_ms, e->prep_ev[0], e->prep_ev[1]));
    return UFM_OK;
}

// ---- reads of the rasters ----
int engine_read_map(Engine *e, int m, uint8_t *host_map) {
    if (!e || !host_map || !e->allocated || m < 0 || m >= e->nmaps) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }
    HIPCHK(hipMemcpyAsync(host_map, e->P.cost + (size_t)m * e->P.cstride, e->P.cstride, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return UFM_OK;
}
int engine_read_raw_map(Engine *e, int m, uint8_t *host_map) {
    if (!e || !host_map || !e->cs.on || !e->allocated || m < 0 || m >= e->nmaps || !e->maps[m].have_map) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(host_map, e->d_raw + (size_t)m * e->P.cstride, e->P.cstride, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return UFM_OK;
}
