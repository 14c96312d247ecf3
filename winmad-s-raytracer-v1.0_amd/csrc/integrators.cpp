#include "integrators.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace winmad {
namespace {
void ok(int rc) {
  if (rc != WR_OK) throw std::runtime_error(std::string("winmad_rt: ") + wr_last_error());
}
}  // namespace

void Parameters::load_parameters(const char* filename) {
  FILE* fp = std::fopen(filename, "r");
  if (!fp) throw std::runtime_error(std::string("cannot open parameter file ") + filename);
  int* slots[8] = {&MAX_TRACING_DEPTH, &SAMPLES_PER_PIXEL, &SAMPLES_OF_LIGHT, &SAMPLES_OF_HEMISPHERE,
                   &WIDTH, &HEIGHT, &PHONG_POWER_INDEX, &POINT_LIGHT_NUM};
  char tok[1024];
  int k = 0;
  while (k < 8 && std::fscanf(fp, "%1023s", tok) == 1) {
    if (tok[0] == '#') continue;  // read_int (parameters.cpp:9-20)
    *slots[k++] = std::atoi(tok);
  }
  for (; k < 8; ++k) *slots[k] = -1;  // read_int returns -1 at EOF
  std::fclose(fp);
}

SurfaceIntegrator::~SurfaceIntegrator() {
  if (ctx_) wr_destroy(ctx_);
  if (scene_) wr_scene_free(scene_);
}

void SurfaceIntegrator::load(const char* filename) {
  ok(wr_scene_load(filename, &scene_));
  if (devices.size() > 1)
    ok(wr_create_multi(scene_, devices.data(), static_cast<int>(devices.size()), &ctx_));
  else
    ok(wr_create(scene_, devices.empty() ? device : devices[0], &ctx_));
  if (traceMode >= 0) ok(wr_set_trace_mode(ctx_, traceMode));
  film.assign(static_cast<size_t>(height) * width * 3, 0.f);
  // the render's GPU work buffers now, as the reference's init allocates its
  // film and vertex arrays before render() (bidirPathTracing.cpp:5-21): the
  // render call then only renders
  if (reserveAtInit) ok(wr_reserve(ctx_, integrator_, width, height));
}

void SurfaceIntegrator::setTraceMode(int mode) {
  ok(wr_set_trace_mode(ctx_, mode));
  traceMode = mode;
}

void SurfaceIntegrator::reserve() { ok(wr_reserve(ctx_, integrator_, width, height)); }

// FNV-1a 64 of the scene's fingerprint and the integrator's settings: what a
// resumed film must have been rendered with, beyond the header's size, kind,
// total and seed
uint64_t SurfaceIntegrator::settingsHash(const std::vector<double>& settings) const {
  uint64_t scene = 0;
  ok(wr_scene_fingerprint(scene_, &scene));
  uint64_t h = 1469598103934665603ull;
  auto mix = [&h](const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  };
  mix(&scene, sizeof scene);
  for (double v : settings) mix(&v, sizeof v);
  return h ? h : 1;  // 0 means "not recorded"
}

template <class Batch>
void SurfaceIntegrator::batched(int kind, int total, uint32_t seed, const std::vector<double>& settings, Batch batch,
                                int every) {
  int done = 0;
  stopped = false;
  const uint64_t fp = settingsHash(settings);
  wr_checkpoint_info want{width, height, kind, 0, total, seed, {uint32_t(fp), uint32_t(fp >> 32)}};
  if (!checkpointPath.empty()) {
    wr_checkpoint_info have{};
    if (FILE* f = std::fopen(checkpointPath.c_str(), "rb")) {  // resume
      std::fclose(f);
      ok(wr_checkpoint_load(checkpointPath.c_str(), &have, nullptr, 0));
      if (have.width != width || have.height != height || have.kind != kind || have.total != total ||
          have.seed != seed)
        throw std::runtime_error("checkpoint " + checkpointPath + " belongs to another render");
      // a film without a fingerprint (written before API v7, or saved with 0)
      // cannot be matched to a scene: refused like a foreign one
      if (have.fingerprint[0] == 0 && have.fingerprint[1] == 0)
        throw std::runtime_error("checkpoint " + checkpointPath +
                                 " carries no scene fingerprint (written before API v7 or without one); "
                                 "delete it to render from the start");
      if (have.fingerprint[0] != want.fingerprint[0] || have.fingerprint[1] != want.fingerprint[1])
        throw std::runtime_error("checkpoint " + checkpointPath +
                                 " was rendered from another scene or with other integrator settings");
      ok(wr_checkpoint_load(checkpointPath.c_str(), &have, film.data(), static_cast<int64_t>(film.size())));
      done = have.done;
    }
  }
  while (done < total) {
    int n = total - done;
    if (checkpointEvery > 0) n = std::min(n, checkpointEvery);
    if (every > 0) n = std::min(n, every);
    if (stopAfter >= 0) n = std::min(n, stopAfter - done);
    if (n <= 0) {
      stopped = true;
      return;
    }
    const bool enough = batch(done, n);
    done += n;
    if (!checkpointPath.empty()) {
      want.done = done;
      ok(wr_checkpoint_save(checkpointPath.c_str(), &want, film.data()));
    }
    if (enough) return;
  }
}

namespace {
// the part of render() the two iteration-based integrators share: a batch is
// rendered by plain(begin, count) or moments(begin, count), then the stop rule
template <class Plain, class Moments>
bool error_batch(SurfaceIntegrator& si, ErrorTarget& et, bool denoise, wr_context* ctx, int begin, int count,
                 Plain plain, Moments moments) {
  if (!(et.errorTarget > 0.0)) {
    if (denoise) moments(begin, count);  // the denoiser needs the squared film too
    else plain(begin, count);
    et.iterationsDone = begin + count;
    return false;
  }
  moments(begin, count);
  et.iterationsDone = begin + count;
  if (et.iterationsDone < 2) return false;
  ok(wr_film_error(ctx, si.film.data(), et.filmSq.data(), si.width, si.height, et.iterationsDone, 0, nullptr,
                   &et.errorInfo));
  return et.errorInfo.rel_stderr <= et.errorTarget;
}
void denoise_begin(SurfaceIntegrator& si, Denoise& dn, int passes) {
  dn.denoised.clear();
  if (!dn.denoise) return;
  if (!si.checkpointPath.empty())
    throw std::runtime_error("denoise cannot be combined with a checkpoint: the file does not carry filmSq");
  if (passes < 2) throw std::runtime_error("denoise needs at least 2 iterations (samples): the variance of one is unknown");
}
void error_begin(SurfaceIntegrator& si, ErrorTarget& et, Denoise& dn, int iterations) {
  et.iterationsDone = 0;
  et.errorInfo = wr_error_info{};
  denoise_begin(si, dn, iterations);
  if (dn.denoise) et.filmSq.assign(si.film.size(), 0.f);
  if (!(et.errorTarget > 0.0)) return;
  if (!si.checkpointPath.empty())
    throw std::runtime_error("errorTarget cannot be combined with a checkpoint: the file does not carry filmSq");
  if (et.errorCheckEvery < 1) throw std::runtime_error("errorCheckEvery must be at least 1");
  et.filmSq.assign(si.film.size(), 0.f);
}
// the feature films in the film's layout, then the filter (host films: the
// library's CPU loop); `passes` is what film / filmSq sum
void denoise_film(SurfaceIntegrator& si, Denoise& dn, wr_context* ctx, const std::vector<float>& filmSq, int passes,
                  int layout) {
  if (!dn.denoise || si.stopped) return;
  if (passes < 2) throw std::runtime_error("denoise needs at least 2 iterations (samples) in the film");
  const size_t nf = si.film.size();
  std::vector<float> normal(nf), position(nf), albedo(nf);
  ok(wr_render_features(ctx, si.width, si.height, layout, normal.data(), albedo.data(), position.data(), nullptr, 0,
                        nullptr));
  dn.denoised.assign(nf, 0.f);
  ok(wr_film_denoise(nullptr, si.film.data(), filmSq.data(), si.width, si.height, passes, normal.data(),
                     position.data(), albedo.data(), &dn.denoiseParams, 0, dn.denoised.data()));
}
void need_denoised(const SurfaceIntegrator& si, const Denoise& dn) {
  if (dn.denoised.size() != si.film.size() || dn.denoised.empty())
    throw std::runtime_error("no denoised film: set denoise before render()");
}
void error_map(SurfaceIntegrator& si, ErrorTarget& et, const char* filename) {
  if (et.filmSq.size() != si.film.size() || et.iterationsDone < 2)
    throw std::runtime_error("no error map: render with errorTarget > 0 and at least 2 iterations first");
  std::vector<float> map(si.film.size());
  wr_error_info info{};
  ok(wr_film_error(nullptr, si.film.data(), et.filmSq.data(), si.width, si.height, et.iterationsDone, 0, map.data(),
                   &info));
  ok(wr_film_write_image(map.data(), si.height, si.width, 1.f, 2.2f, si.height == si.width, filename));
}
}  // namespace

void BidirPathTracing::init(const char* filename, Parameters& para) {
  samplesPerPixel = para.SAMPLES_PER_PIXEL;  // stored, unused by BDPT (:11)
  integrator_ = WR_INTEGRATOR_BDPT;
  height = para.HEIGHT;
  width = para.WIDTH;
  load(filename);
}

void BidirPathTracing::render() {
  error_begin(*this, *this, *this, iterations);
  batched(WR_CKPT_BDPT, iterations, seed, {double(maxPathLength), double(controlLength)}, [&](int begin, int count) {  // :25-26
    wr_bdpt_params p{};
    p.width = width;
    p.height = height;
    p.iterations = count;
    p.iter_begin = begin;
    p.control_length = controlLength;
    p.max_path_length = maxPathLength;
    p.seed = seed;
    p.faithful = 1;
    return error_batch(*this, *this, denoise, ctx_, begin, count,
                       [&](int, int) { ok(wr_render_bdpt(ctx_, &p, film.data(), 0, &stats)); },
                       [&](int, int) { ok(wr_render_bdpt_moments(ctx_, &p, film.data(), filmSq.data(), 0, &stats)); });
  }, errorTarget > 0.0 ? errorCheckEvery : 0);
  denoise_film(*this, *this, ctx_, filmSq, iterationsDone, WR_FILM_BDPT);
}

void BidirPathTracing::outputDenoisedImage(const char* filename) {  // as outputImage
  need_denoised(*this, *this);
  const int n = iterationsDone > 0 ? iterationsDone : iterations;
  ok(wr_film_write_image(denoised.data(), height, width, 1.f / n, 2.2f, height == width, filename));
}

void BidirPathTracing::outputImage(const char* filename) {
  // The reference transposes in place assuming height == width (:31-44);
  // only square films are transposed here (non-square reference output is corrupt).
  const int n = iterationsDone > 0 ? iterationsDone : iterations;
  ok(wr_film_write_image(film.data(), height, width, 1.f / n, 2.2f, height == width, filename));
}

void BidirPathTracing::outputErrorMap(const char* filename) { error_map(*this, *this, filename); }

void VertexCM::init(const char* filename, Parameters& para) {
  samplesPerPixel = para.SAMPLES_PER_PIXEL;  // stored, unused (:9)
  integrator_ = WR_INTEGRATOR_VCM;
  height = para.HEIGHT;
  width = para.WIDTH;
  load(filename);
}

void VertexCM::render() {
  error_begin(*this, *this, *this, iterations);
  batched(WR_CKPT_VCM, iterations, seed, {double(minPathLength), double(maxPathLength), double(baseRadiusFactor), double(radiusAlpha)}, [&](int begin, int count) {
    wr_vcm_params p{};
    p.width = width;
    p.height = height;
    p.iterations = count;
    p.iter_begin = begin;  // the merge radius follows the global iteration index (:53-58)
    p.min_path_length = minPathLength;
    p.max_path_length = maxPathLength;
    p.radius_factor = baseRadiusFactor;
    p.radius_alpha = radiusAlpha;
    p.seed = seed;
    return error_batch(*this, *this, denoise, ctx_, begin, count,
                       [&](int, int) { ok(wr_render_vcm(ctx_, &p, film.data(), 0, &stats)); },
                       [&](int, int) { ok(wr_render_vcm_moments(ctx_, &p, film.data(), filmSq.data(), 0, &stats)); });
  }, errorTarget > 0.0 ? errorCheckEvery : 0);
  denoise_film(*this, *this, ctx_, filmSq, iterationsDone, WR_FILM_BDPT);
}

void VertexCM::outputDenoisedImage(const char* filename) {  // as outputImage
  need_denoised(*this, *this);
  const int n = iterationsDone > 0 ? iterationsDone : iterations;
  ok(wr_film_write_image(denoised.data(), height, width, 1.f / n, 2.2f, height == width, filename));
}

void VertexCM::outputImage(const char* filename) {
  // transpose (square films only, :31-42), scale 1/iterations, gamma 2.2 (:44)
  const int n = iterationsDone > 0 ? iterationsDone : iterations;
  ok(wr_film_write_image(film.data(), height, width, 1.f / n, 2.2f, height == width, filename));
}

void VertexCM::outputErrorMap(const char* filename) { error_map(*this, *this, filename); }

void PathIntegrator::init(const char* filename, Parameters& para) {
  maxTracingDepth = para.MAX_TRACING_DEPTH;
  samplesPerPixel = para.SAMPLES_PER_PIXEL;
  samplesOfLight = para.SAMPLES_OF_LIGHT;
  samplesOfHemisphere = para.SAMPLES_OF_HEMISPHERE;
  integrator_ = WR_INTEGRATOR_PATH;
  height = para.HEIGHT;
  width = para.WIDTH;
  load(filename);
}

void PathIntegrator::render() {
  denoise_begin(*this, *this, samplesPerPixel);
  if (denoise) filmSq.assign(film.size(), 0.f);
  batched(WR_CKPT_PT, samplesPerPixel, seed, {double(maxTracingDepth), double(samplesOfLight), double(samplesOfHemisphere)}, [&](int begin, int count) {
    wr_path_params p{};
    p.width = width;
    p.height = height;
    p.spp = samplesPerPixel;
    p.max_depth = maxTracingDepth;
    p.sample_begin = begin;  // sample k of the stratification grid (surfaceIntegrator.cpp:26-32)
    p.sample_count = count;
    p.seed = seed;
    if (denoise) ok(wr_render_path_moments(ctx_, &p, film.data(), filmSq.data(), 0, &stats));
    else ok(wr_render_path(ctx_, &p, film.data(), 0, &stats));
    return false;
  });
  if (stopped) return;
  denoise_film(*this, *this, ctx_, filmSq, samplesPerPixel, WR_FILM_PT);  // of the sums, before the scale
  const float inv = 1.f / samplesPerPixel;  // film->scale(1.f / samplesPerPixel) (:45)
  for (float& v : film) v = v * inv;
  for (float& v : denoised) v = v * inv;
}

void PathIntegrator::outputDenoisedImage(const char* filename) {  // as outputImage
  need_denoised(*this, *this);
  ok(wr_film_write_image(denoised.data(), height, width, 1.f, 2.2f, 0, filename));
}

void PathIntegrator::raytracing(const wr_ray* rays, int64_t n, float* rgb, int sample) {
  ok(wr_path_radiance(ctx_, rays, n, maxTracingDepth, seed, sample, rgb, &stats));
}

void PathIntegrator::outputImage(const char* filename) {
  ok(wr_film_write_image(film.data(), height, width, 1.f, 2.2f, 0, filename));
}

PhotonIntegrator::~PhotonIntegrator() {
  if (map_) wr_photon_map_free(map_);  // before the base class destroys the context
}

void PhotonIntegrator::init(const char* filename, Parameters& para) {  // photonMap.cpp:7-32
  maxTracingDepth = para.MAX_TRACING_DEPTH;
  samplesPerPixel = para.SAMPLES_PER_PIXEL;
  height = para.HEIGHT;
  width = para.WIDTH;
  reserveAtInit = false;  // wr_reserve knows no photon integrator: the render allocates
  if (devices.size() > 1) throw std::runtime_error("winmad_rt: -pm renders on one GPU (photon maps are single-device)");
  load(filename);
}

void PhotonIntegrator::buildPhotonMap() {
  if (map_) wr_photon_map_free(map_);
  map_ = nullptr;
  wr_photon_map_params p{};
  p.n_caustic = nCausticPhotons;
  p.n_indirect = nIndirectPhotons;
  p.max_path_length = maxPathLength;
  p.max_shots = maxPhotonShot;
  p.seed = seed;
  ok(wr_photon_map_build(ctx_, &p, &map_, &stats));
  ok(wr_photon_map_info_get(map_, &mapInfo));
  nCausticPaths = static_cast<int>(mapInfo.caustic_paths);
  nIndirectPaths = static_cast<int>(mapInfo.indirect_paths);
}

void PhotonIntegrator::render() {
  if (checkpointPath.size()) throw std::runtime_error("winmad_rt: -pm has no checkpoint");
  if (!map_) buildPhotonMap();
  wr_photon_params p{};
  p.width = width;
  p.height = height;
  p.spp = samplesPerPixel;
  p.knn = knnPhotons;
  p.max_sqr_dist = maxSqrDis;
  p.direct_target = directTarget;
  p.seed = seed;
  ok(wr_render_photon(ctx_, map_, &p, film.data(), 0, &stats));
  const float inv = 1.f / samplesPerPixel;  // film->scale(1.f / samplesPerPixel) (surfaceIntegrator.cpp:45)
  for (float& v : film) v = v * inv;
}

void PhotonIntegrator::outputImage(const char* filename) {  // photonMap.cpp:45
  ok(wr_film_write_image(film.data(), height, width, 1.f / 150.f, 2.2f, 0, filename));
}

}  // namespace winmad
