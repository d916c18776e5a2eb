// rt_headless.cpp — headless frame driver over the C ABI: the render()/compute() loop of
// src/main.cpp:763-781 and 553-578 without GLFW/GL.  Per frame it updates the light
// (moving_light, main.cpp:541-551) or the rand buffer (fill_rand_buffer, main.cpp:535-539),
// uploads the header, dispatches the mode's programs, advances the 8-slot ring
// (main.cpp:619) and finally writes the last image as a PPM in place of the GL blit
// (main.cpp:783-797, shader_fragment.glsl): the 8-bit frame of rt_download_rgba8, or with --strips
// of rt_group_download_rgba8, converted on the GPU (rt_present).  With --ppm-size WxH the PPM has that
// size instead, the frame scaled as the reference's blit scales it into its window (GL_LINEAR,
// main.cpp:381-388), on the GPU as well: rt_download_rgba8_scaled / rt_group_download_rgba8_scaled.
//
//   rt_headless [--width W] [--height H] [--objects N] [--spp A] [--mode 1..4] [--frames K]
//               [--scene synthetic|1|5|6|7] [--rectangles 0|1] [--seed S] [--device D] [--ppm out.ppm] [--pipeline 0|1]
//               [--strips G] [--devices d0,d1,...] [--balance ROUNDS] [--ppm-size WxH] [--pick X,Y] [--query-tree 0|1]
//               [--mesh FILE.obj]
// --pick X,Y prints, after the last frame, one line `pick x y ind t nx ny nz`: the closest hit of pixel
// (X, Y)'s primary ray (frame coordinates, row 0 = the bottom row) by rt_trace_pixels at threshold 0.
// --mesh FILE.obj loads a triangle mesh (include/rt/mesh.h, librtrt_mesh.so; the frames do not show it) and
// makes --pick answer for scene and mesh together: rt_trace_pixels, then rt_mesh_trace_rays on the pixel's ray
// from the camera with RT_MESH_MERGE.  The line is then `pick x y ind t nx ny nz prim`: prim the mesh's
// triangle where the mesh is strictly closer (ind is then -1), else -1.
// --rectangles 1 turns rt_set_rectangles on (rt_group_set_rectangles with --strips): rectangles are drawn,
// e.g. the area light of --scene 7 (scene 5 with the rectangle light the reference left commented out).
// --strips G > 1 renders the frame as G row strips through the rt_group_* entry points: strip i
// on device devices[i % #devices] (default, without --devices: every visible device in turn,
// starting at --device), cost-balanced with --balance ROUNDS timed plans (0: equal strips),
// assembled on the first device.  A --devices list naming a device that does not exist, or
// more devices than are visible, is refused with a message.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt/abi.h"
#include "rt/mesh.h"

static int check(int rc, const char* what) {
  if (rc < 0) {
    std::fprintf(stderr, "rt_headless: %s failed: %s (%d)\n", what, rt_strerror(rc), rc);
    std::exit(1);
  }
  return rc;
}

// rgba: the 8-bit frame top row first (rt_download_rgba8 / rt_group_download_rgba8 with top_down),
// converted on the GPU; the PPM drops the alpha byte
static void write_ppm(const char* path, const std::vector<uint8_t>& rgba, int W, int H) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return;
  std::fprintf(f, "P6\n%d %d\n255\n", W, H);
  std::vector<unsigned char> row(3 * (size_t)W);
  for (int r = 0; r < H; ++r) {
    for (int x = 0; x < W; ++x)
      for (int c = 0; c < 3; ++c) row[3 * x + c] = rgba[((size_t)r * W + x) * 4 + c];
    std::fwrite(row.data(), 1, row.size(), f);
  }
  std::fclose(f);
}

// The frame as `strips` row strips over the devices in `devlist` (rt_group_*).
static int run_strips(const rt_config& cfg, std::vector<float>& header, int mode, int frames, int pipeline,
                      int rectangles, int strips, const std::string& devlist, int device, int balance, const std::string& ppm,
                      int ppm_w, int ppm_h) {
  std::vector<int> devs;
  for (size_t p = 0; p < devlist.size();) {
    size_t q = devlist.find(',', p);
    if (q == std::string::npos) q = devlist.size();
    devs.push_back(std::atoi(devlist.substr(p, q - p).c_str()));
    p = q + 1;
  }
  const int ndev = rt_device_count();
  if (ndev <= 0) {
    std::fprintf(stderr, "rt_headless: no HIP device is visible\n");
    return 1;
  }
  if (devs.empty()) {
    for (int k = 0; k < ndev; ++k) devs.push_back((device + k) % ndev);
  } else {
    // (every entry < ndev also bounds the distinct devices by the visible ones)
    for (int d : devs)
      if (d < 0 || d >= ndev) {
        std::fprintf(stderr, "rt_headless: --devices names device %d, but only %d device(s) are visible (0..%d)\n",
                     d, ndev, ndev - 1);
        return 1;
      }
  }
  std::vector<int> sd(strips);
  for (int i = 0; i < strips; ++i) sd[i] = devs[i % devs.size()];
  rt_group* g = nullptr;
  check(rt_group_create(strips, sd.data(), &cfg, nullptr, &g), "rt_group_create (peer access to the first device?)");
  if (pipeline) check(rt_group_enable_pipelining(g, 1), "rt_group_enable_pipelining");
  if (rectangles) check(rt_group_set_rectangles(g, 1), "rt_group_set_rectangles");
  // a frame that ends as a PPM is assembled as 8-bit strips (top row first), not float ones; one
  // scaled to --ppm-size is filtered from the float frame, which 8-bit strips would not assemble
  if (!ppm.empty() && ppm_w == 0) check(rt_group_enable_rgba8(g, 1, 1), "rt_group_enable_rgba8");
  std::vector<double> strip_ms(strips, 0.0);
  if (balance > 0) check(rt_group_balance(g, header.data(), mode, balance, strip_ms.data()), "rt_group_balance");
  std::vector<int> b(strips + 1);
  check(rt_group_bounds(g, b.data()), "rt_group_bounds");
  std::printf("strips:");
  for (int i = 0; i < strips; ++i)
    std::printf(" [%d,%d)@%d%s", b[i], b[i + 1], sd[i], rt_group_strip_copies(g, i) > 0 ? "+copy" : "");
  std::printf("\n");
  auto t0 = std::chrono::steady_clock::now();
  check(rt_group_compute_frames(g, header.data(), mode, 0, frames, 7000, 0), "rt_group_compute_frames");
  check(rt_group_synchronize(g), "rt_group_synchronize");
  double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const int W = cfg.width, H = cfg.height, A = cfg.spp;
  std::printf("%dx%d spp=%d mode=%d %d strips%s: %.3f ms/frame (wall), %.1f Mrays/s\n", W, H, A, mode, strips,
              pipeline ? " pipelined" : "", wall / frames, (double)W * H * (mode <= 2 ? A : 1) * frames / (wall * 1e3));
  if (!ppm.empty() && ppm_w > 0) {
    std::vector<uint8_t> img((size_t)ppm_w * ppm_h * 4);
    check(rt_group_download_rgba8_scaled(g, ppm_w, ppm_h, 1, img.data()), "rt_group_download_rgba8_scaled");
    write_ppm(ppm.c_str(), img, ppm_w, ppm_h);
  } else if (!ppm.empty()) {
    std::vector<uint8_t> img((size_t)W * H * 4);
    check(rt_group_download_rgba8(g, img.data()), "rt_group_download_rgba8");
    write_ppm(ppm.c_str(), img, W, H);
  }
  rt_group_destroy(g);
  return 0;
}

// the file's bytes; exits with a message if it cannot be read
static std::string read_file(const std::string& path) {
  std::string text;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    std::fprintf(stderr, "rt_headless: cannot open %s\n", path.c_str());
    std::exit(1);
  }
  char buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
  std::fclose(f);
  return text;
}

int main(int argc, char** argv) {
  int W = 440, H = 330, N = 5, A = 4, mode = 1, frames = 8, device = 0, pipeline = 0, strips = 1, balance = 0, rectangles = 0, query_tree = 0;
  int ppm_w = 0, ppm_h = 0;  // --ppm-size (0: the frame's own size)
  bool pick = false;         // --pick X,Y: what is under that pixel after the last frame
  int pick_x = 0, pick_y = 0;
  std::string scene = "1", ppm, devlist, mesh_path;
  unsigned long long seed = 1234;
  for (int i = 1; i + 1 < argc; i += 2) {
    std::string k = argv[i], v = argv[i + 1];
    if (k == "--width") W = std::atoi(v.c_str());
    else if (k == "--height") H = std::atoi(v.c_str());
    else if (k == "--objects") N = std::atoi(v.c_str());
    else if (k == "--spp") A = std::atoi(v.c_str());
    else if (k == "--mode") mode = std::atoi(v.c_str());
    else if (k == "--frames") frames = std::atoi(v.c_str());
    else if (k == "--scene") scene = v;
    else if (k == "--seed") seed = std::strtoull(v.c_str(), nullptr, 10);
    else if (k == "--device") device = std::atoi(v.c_str());
    else if (k == "--ppm") ppm = v;
    else if (k == "--pipeline") pipeline = std::atoi(v.c_str());
    else if (k == "--rectangles") rectangles = std::atoi(v.c_str());
    else if (k == "--query-tree") query_tree = std::atoi(v.c_str());  // --pick through the query tree (rt_set_query_tree)
    else if (k == "--strips") strips = std::atoi(v.c_str());
    else if (k == "--devices") devlist = v;
    else if (k == "--mesh") mesh_path = v;
    else if (k == "--balance") balance = std::atoi(v.c_str());
    else if (k == "--ppm-size") {
      if (std::sscanf(v.c_str(), "%dx%d", &ppm_w, &ppm_h) != 2 || ppm_w < 1 || ppm_h < 1 ||
          ppm_w > RT_PRESENT_SCALED_MAX || ppm_h > RT_PRESENT_SCALED_MAX) {
        std::fprintf(stderr, "rt_headless: --ppm-size wants WxH with both in [1, %d]\n", RT_PRESENT_SCALED_MAX);
        return 2;
      }
    }
    else if (k == "--pick") {
      if (std::sscanf(v.c_str(), "%d,%d", &pick_x, &pick_y) != 2) {
        std::fprintf(stderr, "rt_headless: --pick wants X,Y (frame coordinates, row 0 = the bottom row)\n");
        return 2;
      }
      pick = true;
    }
    else { std::fprintf(stderr, "unknown option %s\n", k.c_str()); return 2; }
  }
  if (!mesh_path.empty() && strips > 1) {
    std::fprintf(stderr, "rt_headless: --mesh goes with --pick on one context; it does not go with --strips\n");
    return 2;
  }
  if (pick && strips > 1) {
    std::fprintf(stderr, "rt_headless: --pick asks one context; it does not go with --strips\n");
    return 2;
  }
  const float aspect = (W * 3 == H * 4) ? 1.333333f : 1.777777f;  // main.cpp:39-40
  int S = scene == "synthetic" ? N : 10;
  std::vector<float> header(rt_header_bytes(S, A) / 4, 0.0f);
  if (scene == "synthetic") check(rt_scenegen(header.data(), S, N, A, seed, aspect), "rt_scenegen");
  else check(rt_init_scene(header.data(), S, A, std::atoi(scene.c_str()), aspect), "rt_init_scene");

  rt_config cfg{W, H, S, A, RT_NUM_FRAMES, RT_RECURSION_DEPTH, 0, 0};
  if (strips > 1) return run_strips(cfg, header, mode, frames, pipeline, rectangles, strips, devlist, device, balance, ppm,
                                ppm_w, ppm_h);
  // the mesh's geometry is read (and a malformed file refused) before anything touches the GPU
  std::vector<float> mesh_verts;
  std::vector<int32_t> mesh_tris;
  if (!mesh_path.empty()) {
    const std::string text = read_file(mesh_path);
    int nv = 0, nt = 0, bad_line = 0;
    if (rt_obj_parse(text.data(), text.size(), nullptr, 0, nullptr, 0, &nv, &nt, &bad_line) != RT_OK) {
      std::fprintf(stderr, "rt_headless: %s: line %d is malformed\n", mesh_path.c_str(), bad_line);
      return 1;
    }
    mesh_verts.resize(3 * (size_t)nv);
    mesh_tris.resize(3 * (size_t)nt);
    check(rt_obj_parse(text.data(), text.size(), mesh_verts.data(), nv, mesh_tris.data(), nt, &nv, &nt, &bad_line), "rt_obj_parse");
  }
  rt_ctx* ctx = nullptr;
  check(rt_create(device, &cfg, &ctx), "rt_create");
  rt_mesh* mesh = nullptr;
  if (!mesh_path.empty())
    check(rt_mesh_create(device, mesh_verts.data(), (int)(mesh_verts.size() / 3), mesh_tris.data(), (int)(mesh_tris.size() / 3), &mesh),
          "rt_mesh_create");
  check(rt_enable_timing(ctx, 1), "rt_enable_timing");
  if (pipeline) check(rt_enable_pipelining(ctx, 1, nullptr), "rt_enable_pipelining");
  if (rectangles) check(rt_set_rectangles(ctx, 1), "rt_set_rectangles");
  if (query_tree) check(rt_set_query_tree(ctx, 1), "rt_set_query_tree");
  int frame = 0;
  auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < frames; ++k) {
    if (mode <= 2) check(rt_fill_rand_buffer(header.data(), S, A, 7000 + (uint64_t)k), "fill_rand_buffer");
    else check(rt_moving_light(header.data(), 0), "moving_light");
    check(rt_set_mode(header.data(), frame, (int)header[4 * RT_HDR_MODE + 2]), "set_mode");
    check(rt_upload_header(ctx, header.data(), header.size() * 4), "rt_upload_header");
    frame = check(rt_dispatch(ctx, mode, frame), "rt_dispatch");
  }
  check(rt_synchronize(ctx), "rt_synchronize");
  double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  double total = 0.0;
  for (int p = 1; p < RT_PROG_COUNT; ++p) {
    int n = 0;
    double ms = 0;
    check(rt_kernel_stats(ctx, p, &n, &ms), "rt_kernel_stats");
    if (n) std::printf("program %d: %d launches, %.3f ms avg\n", p, n, ms / n);
    total += ms;
  }
  // pipelined: kernel spans overlap, so the frame rate comes from the wall clock
  double ms_frame = pipeline ? wall / frames : total / frames;
  std::printf("%dx%d spp=%d objects=%d mode=%d%s: %.3f ms/frame (%s), %.1f Mrays/s, wall %.1f ms\n", W, H, A, N,
              mode, pipeline ? " pipelined" : "", ms_frame, pipeline ? "wall" : "kernels",
              (double)W * H * (mode <= 2 ? A : 1) / (ms_frame * 1e3), wall);
  if (!ppm.empty() && ppm_w > 0) {
    std::vector<uint8_t> img((size_t)ppm_w * ppm_h * 4);
    check(rt_download_rgba8_scaled(ctx, ppm_w, ppm_h, 1, img.data()), "rt_download_rgba8_scaled");
    write_ppm(ppm.c_str(), img, ppm_w, ppm_h);
  } else if (!ppm.empty()) {
    std::vector<uint8_t> img((size_t)W * H * 4);
    check(rt_download_rgba8(ctx, 1, img.data()), "rt_download_rgba8");
    write_ppm(ppm.c_str(), img, W, H);
  }
  if (pick) {  // the closest hit of the pixel's primary ray as mode 3 shows it (t > 0): what mouseCallback would pick
    const int32_t xy[2] = {pick_x, pick_y};
    float t = 0.0f, nrm[3] = {0.0f, 0.0f, 0.0f};
    int32_t ind = 0;
    float dir[3] = {0.0f, 0.0f, 0.0f};
    check(rt_trace_pixels(ctx, xy, 1, 0.0f, &t, &ind, nrm, mesh ? dir : nullptr), "rt_trace_pixels");
    if (mesh) {  // the same ray on the mesh, merged: the mesh takes the pixel only where it is strictly closer
      int32_t prim = -1;
      check(rt_mesh_trace_rays(mesh, &header[4 * RT_HDR_CAMERA_LOCATION], dir, 1, RT_MESH_ONE_ORIGIN | RT_MESH_MERGE, 0.0f, &t,
                               &prim, nrm, nullptr), "rt_mesh_trace_rays");
      if (prim >= 0) ind = -1;
      std::printf("pick %d %d %d %.9g %.9g %.9g %.9g %d\n", pick_x, pick_y, (int)ind, t, nrm[0], nrm[1], nrm[2], (int)prim);
    } else {
      std::printf("pick %d %d %d %.9g %.9g %.9g %.9g\n", pick_x, pick_y, (int)ind, t, nrm[0], nrm[1], nrm[2]);
    }
  }
  if (mesh) rt_mesh_destroy(mesh);
  rt_destroy(ctx);
  return 0;
}
