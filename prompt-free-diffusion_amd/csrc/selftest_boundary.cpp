// selftest --boundary: what a dependent kernel boundary costs behind a producer that leaves B bytes of output, per store
// policy (pfd_common.h, gst<POLICY>).  The producer is the library's store shape -- 16-byte chunks, a wave
// writes 1 KB of one contiguous segment, one 256-thread block per CU -- and the consumer is one block that reads 4 KB of
// what the producer wrote last.  Pairs run back to back on one stream, in-stream and as one hipGraph; reported is the
// time per pair and what it adds to the B = 0 pair.
#include "pfd_common.h"
#include "selftest_util.h"

namespace {
constexpr int PB_BLOCKS = 256, PB_T = 256;

template <int POLICY>
__global__ __launch_bounds__(PB_T) void boundary_producer(char* out, long nchunks, unsigned tag) {
  const uint4 v = make_uint4(tag, tag, tag, tag);
  for (long i = (long)blockIdx.x * PB_T + threadIdx.x; i < nchunks; i += (long)PB_BLOCKS * PB_T)
    gst<POLICY>(out + i * 16, v);
}

// 256 threads x 16 bytes = the last 4 KB the producer wrote (B = 0: the first 4 KB of the buffer, written by nobody)
__global__ __launch_bounds__(PB_T) void boundary_consumer(const char* in, long first_chunk, unsigned* sink) {
  const uint4 v = gld<uint4>(in + (first_chunk + threadIdx.x) * 16);
  sink[threadIdx.x] = (v.x & v.y) | (v.z ^ v.w);   // == tag when the chunk holds {tag, tag, tag, tag}
}

struct Arm {
  const char* name;
  void (*producer)(char*, long, unsigned);
};
const Arm ARMS[] = {{"plain", boundary_producer<ST_PLAIN>}, {"sc1", boundary_producer<ST_WT>}, {"nt", boundary_producer<ST_NT>}};
}  // namespace

int bench_boundary(int, char**) {
  const long MB = 1 << 20;
  const long sizes[] = {0, 1 * MB, 4 * MB, 16 * MB, 32 * MB, 64 * MB};
  const int PAIRS = 200;
  Dev<char> buf((size_t)64 * MB);
  Dev<unsigned> sink(PB_T);
  hipStream_t st;
  HIP_OK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
  int bad = 0;
  printf("boundary probe: %d producer -> consumer pairs per figure, us per pair (and minus the B = 0 pair of the same arm)\n", PAIRS);
  for (int graph = 0; graph < 2; ++graph) {
    for (const Arm& arm : ARMS) {
      double base = 0;
      for (long B : sizes) {
        const long nchunks = B / 16, first = nchunks >= PB_T ? nchunks - PB_T : 0;
        unsigned tag = 1;
        auto run = [&] {
          for (int i = 0; i < PAIRS; ++i) {
            ++tag;
            hipLaunchKernelGGL(arm.producer, dim3(PB_BLOCKS), dim3(PB_T), 0, st, buf.p, nchunks, tag);
            hipLaunchKernelGGL(boundary_consumer, dim3(1), dim3(PB_T), 0, st, (const char*)buf.p, first, sink.p);
          }
        };
        float ms = 0;
        if (!graph) {
          run();
          HIP_OK(hipStreamSynchronize(st));
          HIP_OK(hipEventRecord(e0, st)); run(); HIP_OK(hipEventRecord(e1, st));
          HIP_OK(hipEventSynchronize(e1));
        } else {
          hipGraph_t g; hipGraphExec_t ge;
          HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeGlobal));
          run();
          HIP_OK(hipStreamEndCapture(st, &g));
          HIP_OK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
          HIP_OK(hipGraphLaunch(ge, st));
          HIP_OK(hipStreamSynchronize(st));
          HIP_OK(hipEventRecord(e0, st)); HIP_OK(hipGraphLaunch(ge, st)); HIP_OK(hipEventRecord(e1, st));
          HIP_OK(hipEventSynchronize(e1));
          HIP_OK(hipGraphExecDestroy(ge)); HIP_OK(hipGraphDestroy(g));
        }
        HIP_OK(hipEventElapsedTime(&ms, e0, e1));
        HIP_OK(hipGetLastError());
        const double us = ms * 1e3 / PAIRS;
        if (B == 0) base = us;
        // the consumer of the last pair must have seen the last producer's bytes
        int wrong = 0;
        if (B) for (unsigned s : sink.get()) wrong += s != tag;
        bad += wrong != 0;
        printf("boundary %-7s %-5s B = %2ld MB  %7.2f us/pair  %+7.2f us%s\n", graph ? "graph" : "stream", arm.name, B / MB, us, us - base,
               wrong ? "  STALE READ" : "");
        fflush(stdout);
      }
    }
  }
  HIP_OK(hipEventDestroy(e0)); HIP_OK(hipEventDestroy(e1)); HIP_OK(hipStreamDestroy(st));
  return bad ? 1 : 0;
}
