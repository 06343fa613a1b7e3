// The volume's surface as a triangle mesh through the C++ adaptor (dvo::visualization::SurfaceVolume): two frames fused into a
// volume, the volume meshed, saved, restored and meshed again.
//   match      the second frame aligned against the first: the transformation, as returned, is the second frame's pose in the
//              first frame's world
//   integrate  both frames in one call (the anonymous form: nothing is kept, so the volume can be restored)
//   mesh       extractMesh(): vertices, normals and triangles by surface nets
//   restore    download() into a fresh volume's upload(), meshed again: the same mesh, bit for bit
//   ply        writePly() when a path is given
// Prints counts and checksums -- what examples/volume_mesh_example.c prints through the C ABI.  Input files: float32 planes
// without a header, as tests/test_volume_mesh_adaptor.py writes them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dvo_amd/dense_tracking.hpp"
#include "dvo_amd/point_cloud.hpp"

static std::vector<float> read_plane(const char *path, size_t n) {
  std::vector<float> v(n);
  FILE *f = std::fopen(path, "rb");
  if (!f || std::fread(v.data(), sizeof(float), n, f) != n) {
    std::fprintf(stderr, "cannot read %s\n", path);
    std::exit(2);
  }
  std::fclose(f);
  return v;
}

template <typename T>
static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}

int main(int argc, char **argv) {
  if (argc < 11) {
    std::fprintf(stderr, "usage: %s w h fx fy ox oy first_i first_z second_i second_z [surface.ply]\n", argv[0]);
    return 2;
  }
  typedef dvo::core::RgbdImagePyramid Pyramid;
  typedef dvo::visualization::SurfaceVolume Volume;
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  const size_t n = (size_t)w * h;
  dvo::core::IntrinsicMatrix K =
      dvo::core::IntrinsicMatrix::create((float)std::atof(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6]));

  dvo::core::RgbdCameraPyramid camera(w, h, K);
  std::vector<dvo::core::RgbdImagePyramidPtr> frame;
  for (int k = 0; k < 2; ++k) {
    std::vector<float> i = read_plane(argv[7 + 2 * k], n), z = read_plane(argv[8 + 2 * k], n);
    frame.push_back(camera.create(i.data(), z.data()));
  }

  dvo::DenseTracker::Config cfg = dvo::DenseTracker::getDefaultConfig();
  dvo::DenseTracker tracker(cfg);
  dvo::DenseTracker::Result result;
  tracker.match(*frame[0], *frame[1], result);

  Volume volume;
  std::vector<Pyramid *> frames;
  std::vector<dvo::core::AffineTransformd> poses(2);
  poses[0].setIdentity();
  poses[1] = result.Transformation;
  for (int k = 0; k < 2; ++k) frames.push_back(frame[k].get());
  volume.integrate(frames, poses);

  Volume::Mesh mesh;
  volume.extractMesh(mesh);
  std::printf("mesh counts %lld %lld %lld %lld %lld\n", mesh.counts.vertices, mesh.counts.triangles, mesh.counts.open_edges,
              mesh.counts.uncoloured, mesh.counts.flat);
  double sum = 0.0, along = 0.0;
  long long indices = 0;
  for (size_t i = 0; i < mesh.vertices.size(); ++i) sum += mesh.vertices[i].x, along += mesh.normals[3 * i + 2];
  for (size_t i = 0; i < mesh.triangles.size(); ++i) indices += mesh.triangles[i];
  std::printf("mesh checksum %.17g %.17g %lld\n", sum, along, indices);

  std::vector<dvo_amd_volume_voxel> records;
  volume.download(records);
  Volume copy(volume.options());
  copy.upload(records);
  Volume::Mesh again;
  copy.extractMesh(again);
  const bool same = std::memcmp(&mesh.counts, &again.counts, sizeof(mesh.counts)) == 0 && same_bytes(mesh.vertices, again.vertices) &&
                    same_bytes(mesh.normals, again.normals) && same_bytes(mesh.triangles, again.triangles);
  std::printf("restore same %d\n", same ? 1 : 0);
  if (argc > 11) Volume::writePly(argv[11], mesh);
  return 0;
}
