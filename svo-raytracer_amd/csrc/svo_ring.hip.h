// svo_ring.hip.h -- frames in flight behind the boundary (include/svo_hip.h, svo_ring_*): per slot a stream of its own, output
// buffers for up to `frames` consecutive frames, and the events around its last submission.
//
// Included by svo_hip.hip in two places, because the context holds the ring by value and the ring's functions use the context's
// internals (the way svo_group.hip.h does): in front of svo_ctx for the types below, and behind launch_frame, with
// SVO_RING_FUNCTIONS defined, for the functions.
//
// Lifetime: the whole ring has the image's size (its library-owned images are W x H per frame), so it goes with every svo_resize
// (ring_free from free_outputs).  reserved_cus alone is a setting (svo_set_reserved_cus) and lives as long as the context.
#ifndef SVO_RING_FUNCTIONS

struct RingSlot : Planes {        // (the planes: library-owned images, frame after frame)
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipEvent_t e2 = nullptr;      // behind the forward copy of the last submission (svo_ring_forward_slot), made on demand
  void *xcolor = nullptr, *xdepth = nullptr, *xhits = nullptr; uint64_t xstride = 0;   // caller-owned (svo_ring_bind_slot)
  int first_frame = 0, nframes = 0;
  bool used = false;
  FrameVar *d_fvar = nullptr;   // per-frame cameras of the slot's last submission (svo_ring_submit_cams) ...
  FrameVar *h_fvar = nullptr;   // ... their pinned staging copy, and the event behind the copy that last read it
  hipEvent_t fvar_copied = nullptr;
  // svo_ring_forward_slot: after every submission, src -> dst (a peer's memory) and the submission's number -> *fwd_flag
  const void *fwd_src = nullptr; void *fwd_dst = nullptr; uint64_t fwd_bytes = 0; void *fwd_flag = nullptr;
  int fwd_dst_device = -1;      // >= 0: dst lives on that device of THIS process (svo_group_*): a peer copy
  uint32_t *seq_word = nullptr;
};

struct Ring {
  std::vector<RingSlot> slots;
  int frames = 0;              // frames per slot
  uint64_t stride = 0;         // elements between consecutive frames of a library-owned slot
  unsigned next = 0;           // submissions so far: the next one takes slot next % slots.size()
  int reserved_cus = 0;        // CUs per XCD the ring's streams leave free (svo_set_reserved_cus)
};

#else  // SVO_RING_FUNCTIONS

static void ring_free(svo_ctx *c) {
  Ring &r = c->ring;
  for (auto &s : r.slots) {
    free_planes(s);
    if (s.e0) (void)hipEventDestroy(s.e0);
    if (s.e1) (void)hipEventDestroy(s.e1);
    if (s.e2) (void)hipEventDestroy(s.e2);
    if (s.seq_word) (void)hipFree(s.seq_word);
    if (s.d_fvar) (void)hipFree(s.d_fvar);
    if (s.h_fvar) (void)hipHostFree(s.h_fvar);
    if (s.fvar_copied) (void)hipEventDestroy(s.fvar_copied);
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  r.slots.clear();
  c->pb.set.cus_reserved = 0;
  r.frames = 0; r.stride = 0; r.next = 0;
}

// own_images = false: every slot will be bound to caller-owned buffers before its first submission (svo_group_*)
static int ring_create_impl(svo_ctx *c, int slots, int frames_per_slot, int want_hits, bool own_images) {
  if (!c || slots < 1 || slots > 8 || frames_per_slot < 1 || frames_per_slot > 64)
    return fail(c, SVO_E_INVALID, "svo_ring_create: 1..8 slots of 1..64 frames");
  if (c->width <= 0 || c->height <= 0) return fail(c, SVO_E_INVALID, "svo_ring_create: svo_resize not called");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  ring_free(c);
  Ring &r = c->ring;
  const uint64_t stride = (uint64_t)c->width * (uint64_t)c->height;
  if (stride * (uint64_t)frames_per_slot >= (1ull << 32)) return fail(c, SVO_E_INVALID, "svo_ring_create: slot too large for 32-bit output indices");
  r.slots.resize((size_t)slots);
  const size_t n = (size_t)stride * (size_t)frames_per_slot;
  // CU mask of the slots' streams: bit i = CU i / 8 of XCD i % 8 (tools/cumask_probe.hip); the top 8 r bits cleared
  // keep r CUs of every XCD free of persistent waves
  int ncu = 256;
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device);
  std::vector<uint32_t> cumask((size_t)(ncu + 31) / 32, 0xffffffffu);
  const int reserve = std::min(r.reserved_cus * 8, ncu - 8);
  for (int b = ncu - reserve; b < ncu && reserve > 0; b++) cumask[(size_t)b >> 5] &= ~(1u << (b & 31));
  if (ncu & 31) cumask.back() &= (1u << (ncu & 31)) - 1u;
  c->pb.set.cus_reserved = reserve > 0 ? reserve : 0;
  for (auto &s : r.slots) {
    hipError_t e = reserve > 0 ? hipExtStreamCreateWithCUMask(&s.stream, (uint32_t)cumask.size(), cumask.data())
                               : hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&s.e0);
    if (e == hipSuccess) e = hipEventCreate(&s.e1);
    if (e == hipSuccess && own_images) e = alloc_planes(n, want_hits != 0, s);
    if (e == hipSuccess && own_images) e = hipMemset(s.color, 0, n * 4);
    if (e == hipSuccess && own_images) e = hipMemset(s.depth, 0, n * 4);
    if (e == hipSuccess && own_images && want_hits) e = hipMemset(s.hits, 0, n * 16);
    if (e != hipSuccess) {
      ring_free(c);
      return fail(c, SVO_E_HIP, std::string("svo_ring_create: ") + hipGetErrorString(e));
    }
  }
  HIPCHK(c, hipDeviceSynchronize());   // the zeroing above is asynchronous; the slots' streams do not wait for the null stream
  r.frames = frames_per_slot;
  r.stride = stride;
  return SVO_OK;
}

static RingSlot *ring_slot(svo_ctx *c, int slot, const char *who) {
  if (!c) return nullptr;
  if (slot < 0 || slot >= (int)c->ring.slots.size()) {
    (void)fail(c, SVO_E_INVALID, std::string(who) + ": no such slot (svo_ring_create first)");
    return nullptr;
  }
  return &c->ring.slots[(size_t)slot];
}

// The staged host-to-device copy of a submission's per-frame cameras, on the slot's stream, out of a pinned copy that is
// rewritten only once the copy that last read it has run.  Called by persist_launch for launches whose cameras do not travel in
// the table kernel's arguments.  Returns a hipError_t as int.
static int ring_copy_cams(void *target) {
  const Target *t = (const Target *)target;   // (the slot, the host cameras and their count)
  RingSlot *s = t->cams_slot;
  if (!s || !t->cams || !s->d_fvar) return (int)hipErrorInvalidValue;
  hipError_t e = hipEventSynchronize(s->fvar_copied);
  if (e != hipSuccess) return (int)e;
  memcpy(s->h_fvar, t->cams, (size_t)t->batch * sizeof(FrameVar));
  e = hipMemcpyAsync(s->d_fvar, s->h_fvar, (size_t)t->batch * sizeof(FrameVar), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipEventRecord(s->fvar_copied, s->stream);
  return (int)e;
}

// `cams`: null = nframes consecutive frames of the context's camera starting at frame_number (svo_ring_submit); else nframes
// entries, every frame with its own camera and frameNumber (svo_ring_submit_cams)
static int ring_submit(svo_ctx *c, int frame_number, int nframes, const FrameVar *cams, int *slot, const char *who) {
  if (!c) return SVO_E_INVALID;
  Ring &r = c->ring;
  if (r.slots.empty()) return fail(c, SVO_E_INVALID, std::string(who) + ": svo_ring_create first");
  if (nframes < 1 || nframes > r.frames) return fail(c, SVO_E_INVALID, std::string(who) + ": 1..frames_per_slot frames");
  // the cross-frame accumulation blends with what the previous dispatch left in the SAME image (svotrace.comp:712-719); a
  // ring of several slots hands every submission another image, so a continued accumulation would blend with the frame of
  // `slots` submissions ago.  Sequences that start on a fresh image (svo_set_sequence(n, 1)) are whole in one slot.
  if (c->progressive && !c->seq_fresh && r.slots.size() > 1)
    return fail(c, SVO_E_INVALID, std::string(who) + ": a progressive accumulation that continues on the previous image needs a ring of "
                                  "ONE slot (or svo_dispatch); with several slots start every submission fresh: svo_set_sequence(n, 1)");
  HIPCHK(c, hipSetDevice(c->device));
  const int si = (int)(r.next % (unsigned)r.slots.size());
  RingSlot &s = r.slots[(size_t)si];
  if (!s.xcolor && !s.color) return fail(c, SVO_E_INVALID, std::string(who) + ": the slot has no images (bind it first)");
  // the launch's target: this slot's stream, images and frame range; the context's own dispatch state is not touched
  Target t;
  t.stream = s.stream; t.external = true; t.batch = nframes; t.frame_number = frame_number;
  if (s.xcolor) { t.out.color = (uint32_t *)s.xcolor; t.out.depth = (float *)s.xdepth; t.out.hits = (uint4 *)s.xhits; t.frame_stride = s.xstride; }
  else { t.out = s; t.frame_stride = r.stride; }
  memcpy(t.cam, c->cam, sizeof t.cam);
  // the launch shape a ring of several slots gets unless svo_set_tuning named one: kRingWavesPerCu persistent waves per CU
  if (r.slots.size() > 1) t.shape = kRing;
  int rc = SVO_OK;
  hipError_t e = hipSuccess;
  if (cams && nframes == 1) {           // one frame: simply this frame's camera (beam pre-pass and all)
    memcpy(t.cam, cams[0].cam, sizeof t.cam);
    t.frame_number = cams[0].frame_number;
  } else if (cams) {
    // the batch's cameras live in the slot's table on the device.  Launches with row / column tables carry them there inside the
    // table kernel's arguments (up to kCamPack frames); the others get the staged copy of ring_copy_cams, enqueued by the
    // launch itself in front of the first kernel that reads the table.
    if (!s.d_fvar) {
      e = hipMalloc((void **)&s.d_fvar, (size_t)r.frames * sizeof(FrameVar));
      if (e == hipSuccess) e = hipHostMalloc((void **)&s.h_fvar, (size_t)r.frames * sizeof(FrameVar), hipHostMallocDefault);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&s.fvar_copied, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventRecord(s.fvar_copied, s.stream);   // (so that the first wait below has something to wait for)
    }
    t.cams = cams; t.cams_slot = &s;
    t.frame_number = cams[0].frame_number;
  }
  if (e == hipSuccess) e = hipEventRecord(s.e0, s.stream);
  if (e == hipSuccess) rc = launch_frame(c, t, false);
  if (e == hipSuccess && rc == SVO_OK) e = hipEventRecord(s.e1, s.stream);
  if (e == hipSuccess && rc == SVO_OK && s.fwd_dst) {
    // the slot's frames travel to the frame owner behind the launch, on the same stream: a device-to-device copy (SDMA
    // between GPUs: no CU slot needed next to the persistent waves), then the submission's number into the owner's flag
    if (s.fwd_dst_device >= 0 && s.fwd_dst_device != c->device)
      e = hipMemcpyPeerAsync(s.fwd_dst, s.fwd_dst_device, s.fwd_src, c->device, s.fwd_bytes, s.stream);
    else
      e = hipMemcpyAsync(s.fwd_dst, s.fwd_src, s.fwd_bytes, hipMemcpyDeviceToDevice, s.stream);
    if (e == hipSuccess && s.fwd_flag) {
      e = hipMemsetD32Async((hipDeviceptr_t)s.seq_word, (int)(r.next + 1u), 1, s.stream);
      if (e == hipSuccess) e = hipMemcpyAsync(s.fwd_flag, s.seq_word, 4, hipMemcpyDeviceToDevice, s.stream);
    }
    if (e == hipSuccess && s.e2) e = hipEventRecord(s.e2, s.stream);
  }
  if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (rc) return rc;
  s.first_frame = cams ? cams[0].frame_number : frame_number; s.nframes = nframes; s.used = true;
  r.next++;
  if (slot) *slot = si;
  return SVO_OK;
}

// frame k of a slot: base pointers of its three images
static int ring_frame(svo_ctx *c, int slot, int k, const char *who, const uint32_t **col, const float **dep, const uint4 **hit,
                      size_t *elems = nullptr) {
  RingSlot *s = ring_slot(c, slot, who);
  if (!s) return SVO_E_INVALID;
  if (!s->used || k < 0 || k >= s->nframes) return fail(c, SVO_E_INVALID, std::string(who) + ": the slot does not hold that frame");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(s->e1));
  const uint64_t stride = s->xcolor ? s->xstride : c->ring.stride;
  const uint64_t o = (uint64_t)k * stride;
  // a caller-owned slot may hold less than W x H elements per frame (packed stripes of one rank)
  if (elems) *elems = (size_t)std::min<uint64_t>((uint64_t)c->width * (uint64_t)c->height, stride);
  *col = (s->xcolor ? (const uint32_t *)s->xcolor : s->color) + o;
  *dep = (s->xcolor ? (const float *)s->xdepth : s->depth) + o;
  const uint4 *h = s->xcolor ? (const uint4 *)s->xhits : s->hits;
  *hit = h ? h + o : nullptr;
  return SVO_OK;
}

extern "C" {

int svo_ring_create(svo_ctx *c, int slots, int frames_per_slot, int want_hits) {
  return ring_create_impl(c, slots, frames_per_slot, want_hits, true);
}

int svo_set_reserved_cus(svo_ctx *c, int per_xcd) {
  if (!c || per_xcd < 0 || per_xcd > 16) return fail(c, SVO_E_INVALID, "svo_set_reserved_cus: 0..16 CUs per XCD");
  c->ring.reserved_cus = per_xcd;
  return SVO_OK;
}

int svo_ring_destroy(svo_ctx *c) {
  if (!c) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  ring_free(c);
  return SVO_OK;
}

int svo_ring_bind_slot(svo_ctx *c, int slot, void *color, void *depth, void *hits, uint64_t frame_stride) {
  RingSlot *s = ring_slot(c, slot, "svo_ring_bind_slot");
  if (!s) return SVO_E_INVALID;
  if (color && (!depth || frame_stride == 0)) return fail(c, SVO_E_INVALID, "svo_ring_bind_slot: depth buffer and frame stride required");
  if (color && frame_stride * (uint64_t)c->ring.frames >= (1ull << 32)) return fail(c, SVO_E_INVALID, "svo_ring_bind_slot: slot too large for 32-bit output indices");
  s->xcolor = color; s->xdepth = color ? depth : nullptr; s->xhits = color ? hits : nullptr; s->xstride = color ? frame_stride : 0;
  return SVO_OK;
}

int svo_ring_submit(svo_ctx *c, int frame_number, int nframes, int *slot) {
#if SVO_VARIANTS
  static const bool force_cams = getenv("SVO_FORCE_CAMS") && atoi(getenv("SVO_FORCE_CAMS")) != 0;   // A/B: the kCams kernel on a static camera
#else
  const bool force_cams = false;
#endif
  if (force_cams && c && nframes > 1 && nframes <= 64 && !c->use_beam && !c->progressive) {
    FrameVar v[64];
    for (int k = 0; k < nframes; k++) { memcpy(v[k].cam, c->cam, sizeof v[k].cam); v[k].frame_number = frame_number + k; }
    return ring_submit(c, frame_number, nframes, v, slot, "svo_ring_submit");
  }
  return ring_submit(c, frame_number, nframes, nullptr, slot, "svo_ring_submit");
}

int svo_ring_submit_cams(svo_ctx *c, int nframes, const float *cams, const int *frame_numbers, int *slot) {
  if (!c || !cams || !frame_numbers) return fail(c, SVO_E_INVALID, "svo_ring_submit_cams: null array");
  if (nframes < 1 || nframes > 64) return fail(c, SVO_E_INVALID, "svo_ring_submit_cams: 1..frames_per_slot frames");
  FrameVar v[64];
  for (int k = 0; k < nframes; k++) {
    memcpy(v[k].cam, cams + 15 * (size_t)k, sizeof v[k].cam);
    v[k].frame_number = frame_numbers[k];
  }
  return ring_submit(c, frame_numbers[0], nframes, v, slot, "svo_ring_submit_cams");
}

int svo_ring_wait(svo_ctx *c, int slot) {
  RingSlot *s = ring_slot(c, slot, "svo_ring_wait");
  if (!s) return SVO_E_INVALID;
  if (!s->used) return SVO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(s->e1));
  return SVO_OK;
}

int svo_ring_query(svo_ctx *c, int slot, int *done, int *first_frame, int *nframes, float *gpu_ms) {
  RingSlot *s = ring_slot(c, slot, "svo_ring_query");
  if (!s) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  bool fin = true;
  if (s->used) {
    const hipError_t q = hipEventQuery(s->e1);
    if (q == hipErrorNotReady) fin = false;
    else if (q != hipSuccess) return fail(c, SVO_E_HIP, std::string("svo_ring_query: ") + hipGetErrorString(q));
  }
  if (done) *done = fin ? 1 : 0;
  if (first_frame) *first_frame = s->first_frame;
  if (nframes) *nframes = s->used ? s->nframes : 0;
  if (gpu_ms) {
    *gpu_ms = 0.0f;
    if (s->used && fin) HIPCHK(c, hipEventElapsedTime(gpu_ms, s->e0, s->e1));
  }
  return SVO_OK;
}

int svo_ring_read_color(svo_ctx *c, int slot, int k, void *rgba8) {
  const uint32_t *col; const float *dep; const uint4 *hit;
  if (!rgba8) return fail(c, SVO_E_INVALID, "readback: null buffer");
  size_t n = 0;
  int rc = ring_frame(c, slot, k, "svo_ring_read_color", &col, &dep, &hit, &n);
  if (rc) return rc;
  HIPCHK(c, hipMemcpy(rgba8, col, n * 4, hipMemcpyDeviceToHost));
  return SVO_OK;
}
int svo_ring_read_depth(svo_ctx *c, int slot, int k, float *depth) {
  const uint32_t *col; const float *dep; const uint4 *hit;
  if (!depth) return fail(c, SVO_E_INVALID, "readback: null buffer");
  size_t n = 0;
  int rc = ring_frame(c, slot, k, "svo_ring_read_depth", &col, &dep, &hit, &n);
  if (rc) return rc;
  HIPCHK(c, hipMemcpy(depth, dep, n * 4, hipMemcpyDeviceToHost));
  return SVO_OK;
}
int svo_ring_read_hits(svo_ctx *c, int slot, int k, svo_hit *hits) {
  const uint32_t *col; const float *dep; const uint4 *hit;
  if (!hits) return fail(c, SVO_E_INVALID, "readback: null buffer");
  size_t n = 0;
  int rc = ring_frame(c, slot, k, "svo_ring_read_hits", &col, &dep, &hit, &n);
  if (rc) return rc;
  if (!hit) return fail(c, SVO_E_INVALID, "svo_ring_read_hits: the ring was created without hit records");
  HIPCHK(c, hipMemcpy(hits, hit, n * 16, hipMemcpyDeviceToHost));
  return SVO_OK;
}
int svo_ring_read_pixel(svo_ctx *c, int slot, int k, int x, int y, void *rgba8, float *depth, svo_hit *hit) {
  const uint32_t *col; const float *dep; const uint4 *hp;
  if (!c) return SVO_E_INVALID;
  if (x < 0 || y < 0 || x >= c->width || y >= c->height) return fail(c, SVO_E_INVALID, "svo_ring_read_pixel: outside the image");
  int rc = ring_frame(c, slot, k, "svo_ring_read_pixel", &col, &dep, &hp);
  if (rc) return rc;
  const size_t o = (size_t)y * (size_t)c->width + (size_t)x;
  if (rgba8) HIPCHK(c, hipMemcpy(rgba8, col + o, 4, hipMemcpyDeviceToHost));
  if (depth) HIPCHK(c, hipMemcpy(depth, dep + o, 4, hipMemcpyDeviceToHost));
  if (hit) {
    if (!hp) return fail(c, SVO_E_INVALID, "svo_ring_read_pixel: the ring was created without hit records");
    HIPCHK(c, hipMemcpy(hit, hp + o, 16, hipMemcpyDeviceToHost));
  }
  return SVO_OK;
}

int svo_ring_forward_slot(svo_ctx *c, int slot, const void *src, void *dst, uint64_t nbytes, void *flag) {
  RingSlot *s = ring_slot(c, slot, "svo_ring_forward_slot");
  if (!s) return SVO_E_INVALID;
  if (dst && (!src || nbytes == 0)) return fail(c, SVO_E_INVALID, "svo_ring_forward_slot: source and size required");
  HIPCHK(c, hipSetDevice(c->device));
  if (dst && !s->seq_word) HIPCHK(c, hipMalloc((void **)&s->seq_word, 4));
  if (dst && !s->e2) HIPCHK(c, hipEventCreateWithFlags(&s->e2, hipEventDisableTiming));
  s->fwd_dst_device = -1;
  s->fwd_src = dst ? src : nullptr; s->fwd_dst = dst; s->fwd_bytes = dst ? nbytes : 0; s->fwd_flag = dst ? flag : nullptr;
  return SVO_OK;
}

int svo_ring_device_ptrs(svo_ctx *c, int slot, void **color, void **depth, void **hits, uint64_t *frame_stride, void **stream) {
  RingSlot *s = ring_slot(c, slot, "svo_ring_device_ptrs");
  if (!s) return SVO_E_INVALID;
  if (color) *color = s->xcolor ? s->xcolor : (void *)s->color;
  if (depth) *depth = s->xcolor ? s->xdepth : (void *)s->depth;
  if (hits) *hits = s->xcolor ? s->xhits : (void *)s->hits;
  if (frame_stride) *frame_stride = s->xcolor ? s->xstride : c->ring.stride;
  if (stream) *stream = (void *)s->stream;
  return SVO_OK;
}

}  // extern "C"

#endif  // SVO_RING_FUNCTIONS
