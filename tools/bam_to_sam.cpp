// bam_to_sam.cpp -- an inflated BAM stream (header + records) written out as SAM text, one line per
// record, for tools/sam_bench.py: tests/samutil.py does the same in Python, too slowly for
// benchmark sizes.  Floats are printed with %.9g, which reads back to the same binary32.
//
//   g++ -O2 -std=c++17 -o bam_to_sam tools/bam_to_sam.cpp
//   bam_to_sam IN.inflated OUT.sam
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int32_t rd32(const uint8_t* p) {
  return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}

static void num(std::string& o, long long v) {
  char b[24];
  o.append(b, (size_t)snprintf(b, sizeof b, "%lld", v));
}

static long long aux_int(const uint8_t* p, char t) {
  switch (t) {
    case 'c': return (int8_t)p[0];
    case 'C': return p[0];
    case 's': return (int16_t)(p[0] | p[1] << 8);
    case 'S': return (uint16_t)(p[0] | p[1] << 8);
    case 'i': return rd32(p);
    default: return (uint32_t)rd32(p);
  }
}

static int aux_width(char t) { return t == 'c' || t == 'C' ? 1 : t == 's' || t == 'S' ? 2 : 4; }

static void flt(std::string& o, const uint8_t* p) {
  float f;
  memcpy(&f, p, 4);
  char b[32];
  o.append(b, (size_t)snprintf(b, sizeof b, "%.9g", (double)f));
}

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> u;
  {
    std::vector<uint8_t> buf(1 << 22);
    size_t n;
    while ((n = fread(buf.data(), 1, buf.size(), f)) > 0) u.insert(u.end(), buf.data(), buf.data() + n);
    fclose(f);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o || u.size() < 12 || memcmp(u.data(), "BAM\1", 4) != 0) return 2;
  const uint8_t* d = u.data();
  const size_t N = u.size();
  size_t p = 8 + (size_t)rd32(d + 4);
  {
    size_t tl = p - 8;
    while (tl > 0 && d[8 + tl - 1] == 0) tl--;
    fwrite(d + 8, 1, tl, o);
    if (tl > 0 && d[8 + tl - 1] != '\n') fputc('\n', o);
  }
  std::vector<std::string> names;
  const int32_t nref = rd32(d + p);
  p += 4;
  for (int32_t r = 0; r < nref; r++) {
    const int32_t ln = rd32(d + p);
    names.emplace_back((const char*)d + p + 4, (size_t)ln - 1);
    p += 8 + (size_t)ln;
  }
  static const char SEQ[] = "=ACMGRSVTWYHKDBN", CIG[] = "MIDNSHP=X";
  std::string s;
  while (p + 36 <= N) {
    const uint8_t* r = d + p;
    const size_t end = p + 4 + (size_t)rd32(r);
    if (end > N) return 3;
    const int32_t ref = rd32(r + 4), pos = rd32(r + 8), lrn = r[12], mapq = r[13];
    const int32_t ncig = r[16] | r[17] << 8, flag = r[18] | r[19] << 8, lseq = rd32(r + 20);
    const int32_t nr = rd32(r + 24), np = rd32(r + 28), tlen = rd32(r + 32);
    s.clear();
    s.append((const char*)r + 36, (size_t)lrn - 1);
    s += '\t';
    num(s, flag);
    s += '\t';
    s += ref < 0 ? "*" : names[(size_t)ref];
    s += '\t';
    num(s, (long long)pos + 1);
    s += '\t';
    num(s, mapq);
    s += '\t';
    const uint8_t* q = r + 36 + lrn;
    if (ncig == 0) s += '*';
    for (int32_t c = 0; c < ncig; c++, q += 4) {
      const uint32_t op = (uint32_t)rd32(q);
      num(s, op >> 4);
      s += CIG[op & 15];
    }
    s += '\t';
    s += nr < 0 ? "*" : nr == ref ? "=" : names[(size_t)nr];
    s += '\t';
    num(s, (long long)np + 1);
    s += '\t';
    num(s, tlen);
    s += '\t';
    if (lseq == 0) s += '*';
    for (int32_t i = 0; i < lseq; i++) s += SEQ[(q[i >> 1] >> ((i & 1) ? 0 : 4)) & 15];
    q += (lseq + 1) / 2;
    s += '\t';
    bool star = true;
    for (int32_t i = 0; i < lseq; i++) star = star && q[i] == 0xff;
    if (star) s += '*';
    else
      for (int32_t i = 0; i < lseq; i++) s += (char)(q[i] + 33);
    q += lseq;
    while (q + 3 <= d + end) {
      s += '\t';
      s += (char)q[0];
      s += (char)q[1];
      const char t = (char)q[2];
      q += 3;
      if (t == 'A') {
        s += ":A:";
        s += (char)*q++;
      } else if (t == 'Z' || t == 'H') {
        s += ':';
        s += t;
        s += ':';
        while (*q) s += (char)*q++;
        q++;
      } else if (t == 'f') {
        s += ":f:";
        flt(s, q);
        q += 4;
      } else if (t == 'B') {
        const char sub = (char)q[0];
        const int32_t cnt = rd32(q + 1);
        q += 5;
        s += ":B:";
        s += sub;
        for (int32_t k = 0; k < cnt; k++) {
          s += ',';
          if (sub == 'f') flt(s, q), q += 4;
          else num(s, aux_int(q, sub)), q += aux_width(sub);
        }
      } else {
        s += ":i:";
        num(s, aux_int(q, t));
        q += aux_width(t);
      }
    }
    s += '\n';
    fwrite(s.data(), 1, s.size(), o);
    p = end;
  }
  fclose(o);
  return 0;
}
