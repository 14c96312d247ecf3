// wr_tot -- command-line twin of the reference's main() (src/main.cpp:29-97) for
// the GPU integrators:
//     wr_tot <scene> <out.ppm> -bpt|-vcm|-p|-pm [--params FILE] [--iterations N] [--seed S]
//            [--device D | --gpus N | --devices D0,D1,...] [--trace bvh|reference]
//            [--checkpoint FILE [--checkpoint-every N] [--stop-after N]] [--hw-queues N]
//            [--target-error X [--error-every N] [--error-out map.pfm]] [--denoise FILE]
// --denoise FILE: also write the film filtered by the variance-guided denoiser
// (wr_film_denoise with the first-hit feature films) to FILE, beside the normal
// output; needs at least 2 iterations (-p: samples), not with --checkpoint.
// --target-error X (-bpt / -vcm): render in batches of N iterations (default 4)
// and stop at the first batch boundary where the film's relative standard error
// (wr_film_error's rel_stderr) is at most X, or at --iterations; 0 = off.
// Prints `error <rel_stderr> after <n> iterations`; --error-out writes the
// standard-error map.  Not for -p (its samples are strata of one grid, not
// independent passes) and not together with --checkpoint.
// -pm (photon mapping, main.cpp's PhotonIntegrator): [--seed S] [--photons C,I]
// [--knn K]: the caustic and indirect map sizes (10000,100000) and the photons
// per estimate (50); one GPU, samples per pixel from the parameter file.
// --target-error and --denoise are for -bpt, -vcm and -p only, --checkpoint too.
// Parameters come from src/parameters.para relative to the CWD, as in the
// reference (main.cpp:32), unless --params is given.  Writes time.txt like
// main.cpp:93-95 (seconds instead of clock ticks).
//
// Runs at the configuration bench.py measures: 16 hardware queues for the 16
// render pipelines (HIP and the GPU box default to 4; raised here before the
// first HIP call -- no re-exec), and the verified-BVH traversal for triangle
// scenes (--trace reference: the reference's KD walk; scenes with spheres
// always use it).  --gpus / --devices share the render over several GPUs of the
// node (wr_create_multi); --checkpoint resumes an interrupted render.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "integrators.h"

namespace {
std::vector<int> parse_list(const char* s) {
  std::vector<int> v;
  for (const char* p = s; *p;) {
    char* end = nullptr;
    v.push_back(static_cast<int>(std::strtol(p, &end, 10)));
    if (end == p) throw std::runtime_error(std::string("bad device list ") + s);
    p = (*end == ',') ? end + 1 : end;
  }
  return v;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr,
                 "usage: %s <scene> <out.ppm> -bpt|-vcm|-p|-pm [--params F] [--iterations N] [--seed S] "
                 "[--device D | --gpus N | --devices D0,D1,..] [--trace bvh|reference] "
                 "[--checkpoint F [--checkpoint-every N] [--stop-after N]] [--hw-queues N] "
                 "[--target-error X [--error-every N] [--error-out map.pfm]] [--denoise FILE] "
                 "[-pm: --photons C,I --knn K]\n",
                 argv[0]);
    return 2;
  }
  const char* params = "src/parameters.para";
  const char* checkpoint = nullptr;
  const char* error_out = nullptr;
  const char* denoise_out = nullptr;
  double target_error = 0.0;
  bool have_target = false;
  int error_every = 4;
  int iterations = 1, device = 0, gpus = 0, every = 0, stop_after = -1, hw_queues = 16;
  std::vector<int> devices;
  unsigned seed = 5489;
  bool bvh = true;
  std::vector<int> photons;
  int knn = 50;
  const bool pm = !std::strcmp(argv[3], "-pm");
  try {
    for (int i = 4; i + 1 < argc; i += 2) {
      const char* a = argv[i];
      const char* v = argv[i + 1];
      if (!std::strcmp(a, "--params")) params = v;
      else if (!std::strcmp(a, "--iterations")) iterations = std::atoi(v);
      else if (!std::strcmp(a, "--seed")) seed = static_cast<unsigned>(std::strtoul(v, nullptr, 10));
      else if (!std::strcmp(a, "--device")) device = std::atoi(v);
      else if (!std::strcmp(a, "--gpus")) gpus = std::atoi(v);
      else if (!std::strcmp(a, "--devices")) devices = parse_list(v);
      else if (!std::strcmp(a, "--trace")) bvh = std::strcmp(v, "reference") != 0;
      else if (!std::strcmp(a, "--checkpoint")) checkpoint = v;
      else if (!std::strcmp(a, "--checkpoint-every")) every = std::atoi(v);
      else if (!std::strcmp(a, "--stop-after")) stop_after = std::atoi(v);
      else if (!std::strcmp(a, "--hw-queues")) hw_queues = std::atoi(v);
      else if (!std::strcmp(a, "--target-error")) {
        char* end = nullptr;
        target_error = std::strtod(v, &end);
        have_target = true;
        if (end == v || *end || !(target_error >= 0.0))
          throw std::runtime_error(std::string("usage: --target-error takes a number >= 0 (0 = off), not ") + v);
      } else if (!std::strcmp(a, "--error-every")) {
        error_every = std::atoi(v);
        if (error_every < 1) throw std::runtime_error("usage: --error-every takes a number of iterations >= 1");
      } else if (!std::strcmp(a, "--error-out")) error_out = v;
      else if (!std::strcmp(a, "--denoise")) denoise_out = v;
      else if (!std::strcmp(a, "--photons")) photons = parse_list(v);
      else if (!std::strcmp(a, "--knn")) knn = std::atoi(v);
      else throw std::runtime_error(std::string("unknown option ") + a);
    }
    if (pm && (have_target || denoise_out || checkpoint))
      throw std::runtime_error("usage: --target-error, --denoise and --checkpoint are for -bpt, -vcm and -p only, not -pm");
    if (!pm && (!photons.empty() || knn != 50)) throw std::runtime_error("usage: --photons and --knn are for -pm");
    if (pm && ((!photons.empty() && photons.size() != 2) || knn < 1 || knn > 64))
      throw std::runtime_error("usage: --photons takes C,I (caustic, indirect); --knn 1..64");
    if (have_target && !std::strcmp(argv[3], "-p"))
      throw std::runtime_error("usage: --target-error is for -bpt and -vcm: the samples of -p are strata of one "
                               "grid, stopping early would leave part of each pixel unsampled");
    if (target_error > 0.0 && checkpoint)
      throw std::runtime_error("usage: --target-error cannot be combined with --checkpoint "
                               "(the checkpoint file does not carry the squared film)");
    if (error_out && !(target_error > 0.0))
      throw std::runtime_error("usage: --error-out needs --target-error X with X > 0");
    if (denoise_out && checkpoint)
      throw std::runtime_error("usage: --denoise cannot be combined with --checkpoint "
                               "(the checkpoint file does not carry the squared film)");
    if (denoise_out && std::strcmp(argv[3], "-p") && iterations < 2)
      throw std::runtime_error("usage: --denoise needs --iterations of at least 2 (the variance of one is unknown)");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  // before any HIP call: one hardware queue per render pipeline
  if (wr_request_hw_queues(hw_queues) < 0) {
    std::fprintf(stderr, "%s\n", wr_last_error());
    return 2;
  }
  if (gpus > 0 && devices.empty())
    for (int k = 0; k < gpus; ++k) devices.push_back(k);
  try {
    winmad::Parameters para;
    para.load_parameters(params);
    auto t0 = std::chrono::steady_clock::now();
    std::unique_ptr<winmad::SurfaceIntegrator> integ;
    winmad::ErrorTarget* et = nullptr;
    winmad::Denoise* dn = nullptr;
    if (!std::strcmp(argv[3], "-bpt")) {
      auto* b = new winmad::BidirPathTracing();
      b->iterations = iterations;
      b->seed = seed;
      et = b;
      dn = b;
      integ.reset(b);
    } else if (!std::strcmp(argv[3], "-vcm")) {  // main.cpp:53-58
      auto* v = new winmad::VertexCM();
      v->iterations = iterations;
      v->seed = seed;
      et = v;
      dn = v;
      integ.reset(v);
    } else if (!std::strcmp(argv[3], "-p")) {
      auto* p = new winmad::PathIntegrator();
      p->seed = seed;
      dn = p;
      integ.reset(p);
      if (denoise_out && para.SAMPLES_PER_PIXEL < 2) {
        std::fprintf(stderr, "usage: --denoise needs at least 2 samples per pixel (the variance of one is unknown)\n");
        return 2;
      }
    } else if (pm) {
      auto* p = new winmad::PhotonIntegrator();
      p->seed = seed;
      p->knnPhotons = knn;
      if (photons.size() == 2) p->nCausticPhotons = photons[0], p->nIndirectPhotons = photons[1];
      integ.reset(p);
    } else {
      std::printf("error!\n");  // main.cpp:88-91
      return 1;
    }
    if (et) {
      et->errorTarget = target_error;
      et->errorCheckEvery = error_every;
    }
    if (dn) dn->denoise = denoise_out != nullptr;
    integ->device = device;
    integ->devices = devices;
    integ->traceMode = WR_TRACE_REFERENCE;
    if (checkpoint) {
      integ->checkpointPath = checkpoint;
      integ->checkpointEvery = every;
      integ->stopAfter = stop_after;
    }
    integ->init(argv[1], para);
    if (bvh) {  // the verified BVH traversal where the scene allows it (triangles only)
      try {
        integ->setTraceMode(WR_TRACE_BVH);
      } catch (const std::exception&) {
        bvh = false;
      }
    }
    if (!pm) integ->reserve();  // the GPU work buffers, before the render (as init's allocations in the reference)
    integ->render();
    if (integ->stopped) {
      std::printf("stopped after --stop-after %d; checkpoint %s\n", stop_after, checkpoint);
      return 0;
    }
    integ->outputImage(argv[2]);
    if (denoise_out) {
      if (auto* b = dynamic_cast<winmad::BidirPathTracing*>(integ.get())) b->outputDenoisedImage(denoise_out);
      else if (auto* v = dynamic_cast<winmad::VertexCM*>(integ.get())) v->outputDenoisedImage(denoise_out);
      else if (auto* p = dynamic_cast<winmad::PathIntegrator*>(integ.get())) p->outputDenoisedImage(denoise_out);
    }
    if (et && target_error > 0.0) {
      std::printf("error %.6g after %d iterations\n", et->errorInfo.rel_stderr, et->iterationsDone);
      if (error_out) {
        if (auto* b = dynamic_cast<winmad::BidirPathTracing*>(integ.get())) b->outputErrorMap(error_out);
        else if (auto* v = dynamic_cast<winmad::VertexCM*>(integ.get())) v->outputErrorMap(error_out);
      }
    }
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (FILE* f = std::fopen("time.txt", "w")) {
      std::fprintf(f, "time = %.6f s\n", sec);
      std::fclose(f);
    }
    if (auto* p = dynamic_cast<winmad::PhotonIntegrator*>(integ.get())) {
      const wr_photon_map_info& m = p->mapInfo;
      std::printf("photon maps: %lld shots, %d caustic (%lld paths), %d indirect (%lld paths); frame in %.3f s [trace %s]\n",
                  static_cast<long long>(m.shots), m.caustic_count, static_cast<long long>(m.caustic_paths),
                  m.indirect_count, static_cast<long long>(m.indirect_paths), p->stats.seconds, bvh ? "bvh" : "reference");
      return 0;
    }
    const wr_stats& s = integ->stats;
    std::printf("rays %lld (closest %lld, shadow %lld) in %.3f s: %.2f Mrays/s [trace %s, %zu GPU(s)]\n",
                static_cast<long long>(s.closest_rays + s.shadow_rays), static_cast<long long>(s.closest_rays),
                static_cast<long long>(s.shadow_rays), s.seconds,
                (s.closest_rays + s.shadow_rays) / s.seconds * 1e-6, bvh ? "bvh" : "reference",
                devices.size() > 1 ? devices.size() : size_t(1));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
