// loader_check -- odk_model_load on the CPU, without the kernels (make -C open_duck_playground_amd/csrc loader_check).
//
//   loader_check [--dump DIR] [--expect ok|refused] [--truncations STEP] blob.odkm ...
//
// Loads each ODKM blob file (open_duck_playground_amd.model.Model.blob(), written to a file) from a heap buffer of exactly the
// file's size, prints its return code and error string, and with --dump writes DIR/<file name>.bin: the raw bytes of
// odk_model::h (DevModel), then shape, adr_global_linvel, the height field's sample count and its samples -- two builds of the
// loader agree on a model iff the files are equal (cmp).  --expect ok: every blob must load; --expect refused: every blob must
// be refused with ODK_ERR_INVALID or ODK_ERR_UNSUPPORTED (corrupt copies).  --truncations STEP: after a blob, also every copy of it cut
// to 16, 16 + STEP, ... bytes -- ends inside headers, payloads and paddings --, each of which must be refused.  Exit status 1 when one
// is not as expected.
// Built with -fsanitize=address,undefined (make -B loader_check SAN=...) this is the loader's sanitizer run: host code only,
// nothing here touches a GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../open_duck_playground_amd/csrc/odk_host.h"

int main(int argc, char** argv) {
  std::string dump, expect;
  int nbad = 0, nfile = 0, step = 0, ntrunc = 0, nok = 0, ninvalid = 0, nunsupported = 0;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--dump") && i + 1 < argc) { dump = argv[++i]; continue; }
    if (!strcmp(argv[i], "--expect") && i + 1 < argc) { expect = argv[++i]; continue; }
    if (!strcmp(argv[i], "--truncations") && i + 1 < argc) { step = atoi(argv[++i]); continue; }
    FILE* f = fopen(argv[i], "rb");
    if (!f) { fprintf(stderr, "%s: cannot open\n", argv[i]); return 2; }
    fseek(f, 0, SEEK_END);
    const size_t len = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    std::unique_ptr<unsigned char[]> buf(new unsigned char[len ? len : 1]);   // exactly len bytes: a read past the end is a heap overflow
    if (fread(buf.get(), 1, len, f) != len) { fprintf(stderr, "%s: short read\n", argv[i]); return 2; }
    fclose(f);
    odk_model* m = nullptr;
    const int rc = odk_model_load(buf.get(), len, &m);
    nfile++; nok += rc == ODK_OK; ninvalid += rc == ODK_ERR_INVALID; nunsupported += rc == ODK_ERR_UNSUPPORTED;
    const bool good = expect.empty() || (expect == "ok" ? rc == ODK_OK : rc == ODK_ERR_INVALID || rc == ODK_ERR_UNSUPPORTED);
    if (!good || expect != "refused") printf("%s: %d%s%s\n", argv[i], rc, rc ? " " : "", rc ? odk_last_error() : "");
    nbad += !good;
    if (rc == ODK_OK && !dump.empty()) {
      const char* base = strrchr(argv[i], '/');
      const std::string path = dump + "/" + (base ? base + 1 : argv[i]) + ".bin";
      FILE* o = fopen(path.c_str(), "wb");
      if (!o) { fprintf(stderr, "%s: cannot write\n", path.c_str()); return 2; }
      const int32_t tail[3] = {m->shape, m->adr_global_linvel, (int32_t)m->hfield.size()};
      fwrite(&m->h, sizeof(m->h), 1, o);
      fwrite(tail, sizeof(tail), 1, o);
      fwrite(m->hfield.data(), sizeof(float), m->hfield.size(), o);
      fclose(o);
    }
    odk_model_free(m);
    for (size_t cut = 16; step > 0 && cut < len; cut += step) {
      std::unique_ptr<unsigned char[]> part(new unsigned char[cut]);   // a buffer of its own: the bytes behind the cut do not exist
      memcpy(part.get(), buf.get(), cut);
      odk_model* t = nullptr;
      const int rt = odk_model_load(part.get(), cut, &t);
      ntrunc++; ninvalid += rt == ODK_ERR_INVALID; nunsupported += rt == ODK_ERR_UNSUPPORTED;
      if (rt != ODK_ERR_INVALID && rt != ODK_ERR_UNSUPPORTED) { printf("%s cut to %zu bytes: %d\n", argv[i], cut, rt); nbad++; }
      odk_model_free(t);
    }
  }
  printf("loader_check: %d blobs and %d truncations: %d ok, %d ODK_ERR_INVALID, %d ODK_ERR_UNSUPPORTED, %d not as expected\n", nfile, ntrunc, nok, ninvalid, nunsupported, nbad);
  return nbad ? 1 : 0;
}
