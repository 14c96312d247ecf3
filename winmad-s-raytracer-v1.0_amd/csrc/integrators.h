// C++ host mirror of the reference's integrator seam, over the C ABI.
//
// The reference's drop-in point is SurfaceIntegrator
// (src/surfaceIntegrator/surfaceIntegrator.h:14-34): main() picks an integrator by
// flag and calls init(scene, para) / render() / outputImage(path)
// (src/main.cpp:40-45 for -p, :65-70 for -bpt).  These classes keep those names
// and that call order; the work happens on the GPU through include/winmad_rt.h.
// Where the reference would crash (missing scene, no lights) these throw
// std::runtime_error carrying wr_last_error().
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "winmad_rt.h"

namespace winmad {

// src/parameters.h / parameters.cpp:22-34 -- 8 positional ints, '#' lines skipped
class Parameters {
 public:
  int MAX_TRACING_DEPTH = 7, SAMPLES_PER_PIXEL = 1, SAMPLES_OF_LIGHT = 8, SAMPLES_OF_HEMISPHERE = 4;
  int WIDTH = 512, HEIGHT = 512, PHONG_POWER_INDEX = 5, POINT_LIGHT_NUM = 400;
  void load_parameters(const char* filename);
};

class SurfaceIntegrator {
 public:
  int width = 0, height = 0, samplesPerPixel = 0;
  int device = 0;
  std::vector<int> devices;  // more than one: the GPUs of this node share the render (wr_create_multi)
  bool reserveAtInit = true;  // init() allocates the render's work buffers (wr_reserve)
  int traceMode = -1;        // -1: the library's default (WR_TRACE_BVH for triangle scenes); WR_TRACE_REFERENCE / WR_TRACE_BVH
  // Film checkpoint (the reference keeps the film in memory only,
  // bidirPathTracing.cpp:23-27): with a path set, render() resumes from a
  // matching checkpoint and saves one every checkpointEvery iterations
  // (samples) and at the end.  stopAfter >= 0 stops once that many are done
  // (an interruption, for tests); `stopped` then says the film is partial.
  std::string checkpointPath;
  int checkpointEvery = 0;
  int stopAfter = -1;
  bool stopped = false;
  std::vector<float> film;  // ImageFilm color[height][width] (r, g, b)
  wr_stats stats{};
  virtual ~SurfaceIntegrator();
  virtual void init(const char* filename, Parameters& para) = 0;
  virtual void render() = 0;
  virtual void outputImage(const char* filename) = 0;
  // wr_set_trace_mode after init (throws, e.g. WR_TRACE_BVH on a scene with spheres)
  void setTraceMode(int mode);
  // wr_reserve after init / setTraceMode: the render's GPU buffers now, so that
  // render() only renders (init() already does it unless reserveAtInit is false;
  // render() allocates whatever is missing otherwise)
  void reserve();

 protected:
  int integrator_ = WR_INTEGRATOR_BDPT;  // set by init: what reserve() allocates for
  wr_scene* scene_ = nullptr;
  wr_context* ctx_ = nullptr;
  void load(const char* filename);
  // the render loop in batches: renders [done, total) through batch(begin, count),
  // resuming from / saving checkpoints of `kind`
  // (every > 0: batches of at most `every`; a batch that returns true ends the render)
  template <class Batch>
  void batched(int kind, int total, uint32_t seed, const std::vector<double>& settings, Batch batch, int every = 0);
  // hash of the scene (wr_scene_fingerprint) and `settings`: stored in the
  // checkpoint, a resume with another scene or settings is refused
  uint64_t settingsHash(const std::vector<double>& settings) const;
};

// Noise-target stopping of the iteration-based integrators (no reference
// counterpart; winmad_rt.h, second-moment films).  With errorTarget > 0,
// render() runs wr_render_*_moments in batches of errorCheckEvery iterations,
// asks wr_film_error after each and stops at the first batch boundary where
// rel_stderr <= errorTarget, or at `iterations`.  iterationsDone is what the
// film holds; outputImage scales by 1 / iterationsDone.  Not combined with a
// checkpoint (the file does not carry filmSq): render() throws.
class ErrorTarget {
 public:
  double errorTarget = 0.0;  // 0 = off: render() is the plain render
  int errorCheckEvery = 4;   // iterations per batch
  int iterationsDone = 0;
  wr_error_info errorInfo{};  // of the last check (zero before the second iteration)
  std::vector<float> filmSq;  // sum of the squared iteration films (errorTarget > 0, or Denoise::denoise)
};

// The film denoiser (no reference counterpart; winmad_rt.h wr_film_denoise).
// With `denoise` set, render() keeps the squared film too -- it goes through the
// moments call even without an errorTarget -- and, once the film is complete,
// renders the first-hit feature films in the integrator's film layout and
// filters the film with them: `denoised` is a film like `film`, and
// outputDenoisedImage writes it exactly as outputImage writes `film`.  Needs at
// least 2 iterations (samples); not combined with a checkpoint (the file does
// not carry the squared film): render() throws.
class Denoise {
 public:
  bool denoise = false;
  wr_denoise_params denoiseParams{5, 7, 4.f, 0.05f, 0.1f};
  std::vector<float> denoised;
};

// src/surfaceIntegrator/bidirPathTracing.{h,cpp}
class BidirPathTracing : public SurfaceIntegrator, public ErrorTarget, public Denoise {
 public:
  void outputDenoisedImage(const char* filename);
  // the standard-error map of the film (errorTarget > 0, >= 2 iterations), as
  // outputImage writes the film: transposed when square; .pfm keeps the floats
  void outputErrorMap(const char* filename);
  int minPathLength = 0, maxPathLength = 10, controlLength = 3;
  int iterations = 1;  // bidirPathTracing.cpp:9
  uint32_t seed = 5489;
  void init(const char* filename, Parameters& para) override;  // :5-21
  void render() override;                                        // :23-27
  void outputImage(const char* filename) override;               // :29-46
};

// src/surfaceIntegrator/vertexcm.{h,cpp}
class VertexCM : public SurfaceIntegrator, public ErrorTarget, public Denoise {
 public:
  void outputDenoisedImage(const char* filename);
  void outputErrorMap(const char* filename);
  int minPathLength = 0, maxPathLength = 10;
  int iterations = 1;            // vertexcm.cpp:7
  float baseRadiusFactor = 0.003f;  // baseRadius = 0.003 * sceneRadius (:13)
  float radiusAlpha = 0.75f;     // :14
  uint32_t seed = 5489;
  void init(const char* filename, Parameters& para) override;  // :3-21
  void render() override;                                        // :23-27
  void outputImage(const char* filename) override;               // :29-45
};

// src/surfaceIntegrator/pathIntegrator.{h,cpp} + SurfaceIntegrator::render
class PathIntegrator : public SurfaceIntegrator, public Denoise {
 public:
  void outputDenoisedImage(const char* filename);
  std::vector<float> filmSq;  // sum of the squared sample films (denoise)
  int maxTracingDepth = 7, samplesOfLight = 8, samplesOfHemisphere = 4;
  uint32_t seed = 5489;
  void init(const char* filename, Parameters& para) override;  // pathIntegrator.cpp:3-15
  void render() override;                                        // surfaceIntegrator.cpp:14-46
  void outputImage(const char* filename) override;               // surfaceIntegrator.cpp:47-50
  // raytracing(const Ray&, int dep) (pathIntegrator.cpp:29-148) for a batch of
  // rays; rgb: n * 3 radiance values (dep is unused by the reference)
  void raytracing(const wr_ray* rays, int64_t n, float* rgb, int sample = 0);
};

// src/surfaceIntegrator/photonMap.{h,cpp} + SurfaceIntegrator::render.  One GPU;
// no checkpoint, error target or denoiser.  render() builds the maps first
// if buildPhotonMap() has not been called.
class PhotonIntegrator : public SurfaceIntegrator {
 public:
  int nCausticPhotons = 10000, nIndirectPhotons = 100000, knnPhotons = 50;  // photonMap.cpp:9-19
  float maxSqrDis = 0.1f;
  int maxPathLength = 5, maxPhotonShot = 500000;  // (the cap holds here: the reference never reads it)
  int nCausticPaths = 0, nIndirectPaths = 0;
  int maxTracingDepth = 7;
  int directTarget = 0;  // 0: the reference's direct-light shadow ray (photonMap.cpp:259); 1: to the light
  uint32_t seed = 5489;
  wr_photon_map_info mapInfo{};
  ~PhotonIntegrator() override;
  void init(const char* filename, Parameters& para) override;  // :7-32
  void buildPhotonMap();                                         // :48-162
  void render() override;                                        // surfaceIntegrator.cpp:14-46 over :304-366
  void outputImage(const char* filename) override;               // :34-46: scale 1 / 150, gamma 2.2

 private:
  wr_photon_map* map_ = nullptr;
};

}  // namespace winmad
