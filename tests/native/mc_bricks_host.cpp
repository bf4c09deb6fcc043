// Host build of the brick marching cubes' per-point statements (vqnerf_release_amd/csrc/mc_bricks_core.h, the text the kernels of
// marching_cubes_bricks.hip loop over a brick's points): the same loops, one brick after the other, as plain C++.
//  * as a shared library (tests/test_mesh_bricks_native.py): h_classify / h_emit against the NumPy model of the dense mesher;
//  * with -DMC_BRICKS_MAIN as a stand-alone program under ASan / UBSan: a noise field on a grid with clipped bricks, heap arrays of
//    the exact sizes, the full brick list and lists with one brick left out (the leak path: counted, every index in range).
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "mc_table.h"
#include "mc_bricks_core.h"
static BrickGrid grid(int nx,int ny,int nz){BrickGrid g;g.nx=nx;g.ny=ny;g.nz=nz;g.nbx=(nx+6)/8;g.nby=(ny+6)/8;g.nbz=(nz+6)/8;return g;}
extern "C" void h_classify(const float* ub,const int32_t* ijk,int n,const int32_t* slot,int nx,int ny,int nz,float thr,int32_t* vc,int32_t* tc,int64_t* keys,int32_t* leaks){
  BrickGrid g=grid(nx,ny,nz); *leaks=0;
  for(int s=0;s<n;++s){Brick k; bool ok=brk_brick(g,ijk+3*s,&k); const float* u=ub+(long)s*729; int face[12]={0};
    for(int l=0;l<729;++l){int nv=0,nt=0;int64_t key=VQN_BRK_NOKEY; if(ok){brk_classify_point(u,g,k,l,thr,&nv,&nt,&key);
      int lk=l%9,lj=(l/9)%9,li=l/81; if(li<k.x.ns&&lj<k.y.ns&&lk<k.z.ns){int in=brk_inside(u[l],thr);
       if(li==0)face[0+in]=1; if(li==k.x.ns-1)face[2+in]=1; if(lj==0)face[4+in]=1; if(lj==k.y.ns-1)face[6+in]=1; if(lk==0)face[8+in]=1; if(lk==k.z.ns-1)face[10+in]=1;}}
      vc[s*729+l]=nv;tc[s*729+l]=nt;keys[s*729+l]=key;}
    if(ok) for(int t=0;t<6;++t) if(face[2*t]&&face[2*t+1]){int a=t>>1,d=(t&1)?1:-1; int bi=k.x.b+(a==0?d:0),bj=k.y.b+(a==1?d:0),bk=k.z.b+(a==2?d:0);
      if(bi>=0&&bi<g.nbx&&bj>=0&&bj<g.nby&&bk>=0&&bk<g.nbz){int sm=slot[((long)bi*g.nby+bj)*g.nbz+bk]; if(sm<0||sm>=n)(*leaks)++;}}
  }}
extern "C" void h_emit(const float* ub,const int32_t* ijk,int n,const int32_t* slot,int nx,int ny,int nz,float thr,const int32_t* voff,const int32_t* toff,int nv,int nt,const float* org,const float* st,float* verts,int32_t* tris){
  BrickGrid g=grid(nx,ny,nz); BrickOut o; o.voff=voff;o.toff=toff;o.n_verts=nv;o.n_tris=nt;o.ox=org[0];o.oy=org[1];o.oz=org[2];o.stx=st[0];o.sty=st[1];o.stz=st[2];o.verts=verts;o.tris=tris;
  for(int s=0;s<n;++s){Brick k; if(!brk_brick(g,ijk+3*s,&k))continue; for(int l=0;l<729;++l) brk_emit_point(ub+(long)s*729,ub,slot,n,g,k,s,l,thr,o);}
}

#ifdef MC_BRICKS_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <numeric>
#include <vector>
int main(){
  const int nx=19,ny=10,nz=27; BrickGrid g=grid(nx,ny,nz); const float thr=0.5f;
  std::vector<float> u((size_t)nx*ny*nz); unsigned s=12345; for(auto& v:u){s=s*1664525u+1013904223u; v=(s>>8)/16777216.0f;}
  for(int drop=-1; drop<g.nbx*g.nby*g.nbz; drop+=5){
    std::vector<int32_t> ijk; std::vector<int32_t> slot((size_t)g.nbx*g.nby*g.nbz,-1); int n=0;
    for(int bi=0;bi<g.nbx;++bi)for(int bj=0;bj<g.nby;++bj)for(int bk=0;bk<g.nbz;++bk){int lin=(bi*g.nby+bj)*g.nbz+bk; if(lin==drop)continue; slot[lin]=n++; ijk.push_back(bi);ijk.push_back(bj);ijk.push_back(bk);}
    float* ub=(float*)malloc(sizeof(float)*n*729);
    for(int b=0;b<n;++b)for(int l=0;l<729;++l){int i=ijk[3*b]*8+l/81,j=ijk[3*b+1]*8+(l/9)%9,k=ijk[3*b+2]*8+l%9; ub[b*729+l]=(i<nx&&j<ny&&k<nz)?u[((size_t)i*ny+j)*nz+k]:NAN;}
    int32_t* vc=(int32_t*)malloc(4*n*729),*tc=(int32_t*)malloc(4*n*729); int64_t* keys=(int64_t*)malloc(8*n*729); int32_t leaks;
    h_classify(ub,ijk.data(),n,slot.data(),nx,ny,nz,thr,vc,tc,keys,&leaks);
    std::vector<int> order(n*729); std::iota(order.begin(),order.end(),0); std::stable_sort(order.begin(),order.end(),[&](int a,int b){return keys[a]<keys[b];});
    int32_t* voff=(int32_t*)malloc(4*n*729),*toff=(int32_t*)malloc(4*n*729); long nv=0,nt=0;
    for(int o:order){voff[o]=nv;toff[o]=nt;nv+=vc[o];nt+=tc[o];}
    float* verts=(float*)malloc(12*nv); int32_t* tris=(int32_t*)malloc(12*nt); float org[3]={0,0,0},st[3]={1,1,1};
    h_emit(ub,ijk.data(),n,slot.data(),nx,ny,nz,thr,voff,toff,(int)nv,(int)nt,org,st,verts,tris);
    int bad=0; for(long t=0;t<3*nt;++t) if(tris[t]<0||tris[t]>=nv)++bad;
    printf("drop %d: bricks %d verts %ld tris %ld leaks %d bad %d\n",drop,n,nv,nt,leaks,bad);
    if(bad|| (drop<0&&leaks) || (drop>=0&&!leaks)) return 1;
    free(ub);free(vc);free(tc);free(keys);free(voff);free(toff);free(verts);free(tris);
  }
  puts("bricks ok"); return 0;
}
#endif
